"""The flight log without a device (include/lscqp.h, "the flight log"): the numpy restatement (tests/flight_log_reference.py) against quintics
known in power form, the layout's index functions, the exported names, and the shim's writer against the reference's own log lines."""
import ctypes as C
import os
import subprocess
from fractions import Fraction
from math import comb

import numpy as np

from tests import flight_log_reference as FL
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 63, 64, 65, 257)


def _quintics(rng, n, dim, M):
    """Power-form coefficients a[n][dim][M][6] in NORMALISED segment time, multiples of 10/8: the Bernstein control points
    c_i = sum_{j <= i} C(i,j)/C(5,j) a_j (denominators 1, 5, 10) are then dyadic with a few bits -- exact in float32."""
    units = rng.integers(-16, 17, (n, dim, M, 6))  # a_j = units_j * 10 / 8
    c8 = np.zeros_like(units)                       # 8 c_i, an integer: 10 C(i,j) / C(5,j) is one
    for i in range(6):
        for j in range(i + 1):
            w = Fraction(10 * comb(i, j), comb(5, j))
            assert w.denominator == 1
            c8[..., i] += units[..., j] * int(w)
    a, c = units * 1.25, c8 / 8.0
    assert np.array_equal(c.astype(np.float32).astype(np.float64), c)
    return a, c


def _power_form(a, tn, dt):
    """p, p', p'' in real time of sum_j a_j tn^j (tn = normalised time, d/dt = (1/dt) d/dtn); dyadic inputs: exact in float64."""
    p = sum(a[..., j] * tn ** j for j in range(6))
    v = sum(j * a[..., j] * tn ** (j - 1) for j in range(1, 6)) / dt
    acc = sum(j * (j - 1) * a[..., j] * tn ** (j - 2) for j in range(2, 6)) / dt ** 2
    return p, v, acc


def test_known_quintics_in_a_segment_at_zero_on_a_boundary_and_beyond_the_horizon():
    """dt = 0.25, M = 4 (horizon 1.0), dim 3 and dim 2.  record_time_step 0.3125: samples at 0, inside segments 1, 2 and 3 (normalised time
    0.25, 0.5, 0.75) and at 1.25 beyond the horizon (the last control point, tn = 1).  record_time_step 0.25: every sample exactly on a
    segment boundary -- the NEXT segment at tn = 0 -- then t = M dt and beyond.  Position, velocity and acceleration of the restatement
    within one float32 ulp of the polynomial's p, p', p''."""
    M, dt, z = 4, 0.25, 0.6
    rng = np.random.default_rng(17)
    for dim in (3, 2):
        a, c = _quintics(rng, 7, dim, M)
        x = c.reshape(7, dim * M * 6)
        for rts, S, where in ((0.3125, 5, [(0, 0.0), (1, 0.25), (2, 0.5), (3, 0.75), (3, 1.0)]),
                              (0.25, 6, [(0, 0.0), (1, 0.0), (2, 0.0), (3, 0.0), (3, 1.0), (3, 1.0)])):
            got = FL.states_f64(x, M, dim, dt, S, rts, z)
            assert got.shape == (7, S, 9)
            for s, (ms, tn) in enumerate(where):
                assert FL.segment_of(s * rts, M, dt) == (ms, tn)
                want = np.stack(_power_form(a[:, :, ms, :], tn, dt), axis=1)  # (n, 3 kinds, dim)
                for kind in range(3):
                    g, w = got[:, s, 3 * kind:3 * kind + dim], want[:, kind, :]
                    assert (np.abs(g - w) <= np.spacing(np.abs(w).astype(np.float32)).astype(np.float64)).all(), (dim, rts, s, kind)
                if dim == 2:
                    assert (got[:, s, 2] == float(np.float32(z))).all() and not got[:, s, 5].any() and not got[:, s, 8].any()
    # the control points are narrowed to float32 first: a plan that is not float32-exact is evaluated at its float32 neighbours
    x = np.full((1, 3 * M * 6), 0.1)
    assert FL.states_f64(x, M, 3, dt, 1, 0.1, z)[0, 0, 0] == float(np.float32(0.1))


def test_every_slot_of_the_layout_is_distinct_and_inside_its_missions_block():
    """Missions of 1, 63, 64, 65 and 257 agents, S = 3, C = 3, n_dyn = 2: the index functions map every (k, r, a, s) to nine floats of their
    own inside mission k's block of the states buffer, every (k, r, a) to a flags word of its own inside the mission's block, every
    (k, r, oi) to four floats of their own -- and together they fill the three buffers exactly."""
    off = np.concatenate([[0], np.cumsum(SIZES)])
    S, Cap, nd = 3, 3, 2
    n_st, n_fl, n_ob = FL.sizes(off, S, Cap, nd)
    st, fl, ob = np.zeros(n_st, np.int32), np.zeros(n_fl, np.int32), np.zeros(n_ob, np.int32)
    for k in range(len(SIZES)):
        lo, hi = FL.state_block(off, k, S, Cap)
        flo, fhi = FL.flag_block(off, k, Cap)
        assert hi - lo == Cap * SIZES[k] * S * 9 and fhi - flo == Cap * SIZES[k]
        for r in range(Cap):
            for a in range(int(off[k]), int(off[k + 1])):
                f = FL.flag_index(off, k, r, a, Cap)
                assert flo <= f < fhi
                fl[f] += 1
                for s in range(S):
                    i = FL.state_index(off, k, r, a, s, S, Cap)
                    assert lo <= i and i + 9 <= hi
                    st[i:i + 9] += 1
            for oi in range(nd):
                o = FL.obstacle_index(k, r, oi, nd, Cap)
                ob[o:o + 4] += 1
    assert (st == 1).all() and (fl == 1).all() and (ob == 1).all()
    # one mission's block as the download hands it over: [r][a - off[k]][s][9]
    v = FL.mission_views(off, 3, S, Cap, nd, np.arange(n_st), np.arange(n_fl), np.arange(n_ob))
    assert v[0][2, 5, 1, 0] == FL.state_index(off, 3, 2, int(off[3]) + 5, 1, S, Cap) and v[1][2, 5] == FL.flag_index(off, 3, 2, int(off[3]) + 5, Cap)
    assert v[2][1, 1, 0] == FL.obstacle_index(3, 1, 1, nd, Cap)


def test_flags_word():
    w = FL.flags_word([0, 1, 0, 0, 0, 3], [1, 1, 0, 1, 1, 0], [0, 0, 0, 2, 0, 1], [1, 1, 1, 1, 0, 0], [0, 0, 0, 0, 0, 5])
    assert w.tolist() == [0, 1, 2, 4, 8, 31] and w.dtype == np.int32
    assert FL.flags_word([1], [1], [0], [1]).tolist() == [1]


def test_exported_names_prototypes_and_null_refusals(api):
    """The six entries are declared in include/lscqp.h, named in EXPORTED_SYMBOLS and exported; their prototypes are the header's; a NULL
    record or plan is refused before any device is touched; the Python constants are the header's."""
    L = api.lib()
    names = ("lscqp_record_set_log", "lscqp_record_log_obstacles", "lscqp_record_log", "lscqp_record_log_rows", "lscqp_record_log_download",
             "lscqp_plan_set_flight_log")
    for name in names:
        assert name in api.EXPORTED_SYMBOLS and hasattr(L, name), name
    assert L.lscqp_record_set_log.argtypes == [C.c_void_p, C.c_int32, C.c_int32] and L.lscqp_record_set_log.restype is C.c_int
    assert L.lscqp_record_log.restype is C.c_void_p and L.lscqp_record_log.argtypes == [C.c_void_p, C.c_int32, C.c_void_p]
    assert L.lscqp_record_log_download.argtypes == [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    assert L.lscqp_plan_set_flight_log.argtypes == [C.c_void_p, C.c_int32]
    INVALID = api.ERR_INVALID_ARGUMENT
    assert L.lscqp_record_set_log(None, 3, 0) == INVALID and L.lscqp_last_error().decode() == "null record"
    assert L.lscqp_record_log_obstacles(None, None) == INVALID
    assert L.lscqp_record_log_rows(None, None, None) == INVALID
    assert L.lscqp_record_log_download(None, 0, 0, 0, None, None, None) == INVALID
    nb = C.c_uint64(7)
    assert L.lscqp_record_log(None, 0, C.byref(nb)) is None and nb.value == 0
    assert L.lscqp_plan_set_flight_log(None, 3) == INVALID and L.lscqp_last_error().decode() == "null plan"
    hdr = open(os.path.join(ROOT, "include", "lscqp.h")).read()
    for name, val in (("LOG_STATES", 0), ("LOG_FLAGS", 1), ("LOG_OBSTACLES", 2), ("LOG_FLAG_QP_FAILED", 1), ("LOG_FLAG_INVALID", 2),
                      ("LOG_FLAG_GOAL_FAILED", 4), ("LOG_FLAG_SFC_KEPT", 8), ("LOG_FLAG_WAYPOINT", 16)):
        assert getattr(api, name) == val and ("#define LSCQP_%s %d" % (name, val)) in hdr, name
    assert (FL.FLAG_QP_FAILED, FL.FLAG_INVALID, FL.FLAG_GOAL_FAILED, FL.FLAG_SFC_KEPT, FL.FLAG_WAYPOINT) == (1, 2, 4, 8, 16)


def test_shim_writes_a_downloaded_log_as_the_references_lines(tmp_path):
    """SimulationResultCsv::writeFlight (shim/include/result_csv.hpp) from a small host program: the logged positions, velocities and
    accelerations of the reference's first two replans (10 agents, S = 2), arranged as lscqp_record_log_download hands a mission's log
    over, with the fixture's planning times, give the log's header and first three rows character for character."""
    g = H.load_golden("sim_log_states")
    pos, vel, acc = (np.array(g[f], np.float64) for f in ("pos", "vel", "acc"))
    N, S, R = 10, 2, 2
    states = np.zeros((R, N, S, 9), np.float32)
    for r in range(R):
        for s in range(S):
            states[r, :, s, 0:3], states[r, :, s, 3:6], states[r, :, s, 6:9] = pos[2 * r + s], vel[2 * r + s], acc[2 * r + s]
    pt = np.array([g["planning_time"][0], g["planning_time"][2]])  # (rows 0 and 1 are replan 0's, row 2 is replan 1's)
    assert g["planning_time"][0] == g["planning_time"][1]
    src = tmp_path / "log.txt"
    with open(src, "w") as f:
        f.write("%d 0 %d %d 0 0.2 0.1\n" % (N, R, S))
        f.write(" ".join(repr(float(v)) for v in states.reshape(-1)) + "\n")
        f.write(" ".join(repr(float(v)) for v in pt.reshape(-1)) + "\n")
    shim = os.path.join(ROOT, "lsc_dr_planner_amd", "shim")
    exe = tmp_path / "flight_log_csv"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(shim, "include"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(shim, "test", "flight_log_csv.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe), str(src)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == 1 + R * S and lines[:4] == g["raw_lines"]
    assert lines[4].split(",")[1] == "0.3"  # row (1, 1) stands at 1 * time_step + 1 * record_time_step


def test_the_tools_writer_gives_the_same_lines(tmp_path):
    """tools/closed_loop.py: write_flight_csv, the Python twin of the shim's writer (printf's %g is std::ostream's default formatting): the
    same downloaded log gives the reference's header and first three rows character for character; obstacle columns follow the agents'."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import closed_loop

    g = H.load_golden("sim_log_states")
    pos, vel, acc = (np.array(g[f], np.float64) for f in ("pos", "vel", "acc"))
    states = np.zeros((2, 10, 2, 9), np.float32)
    for r in range(2):
        for s in range(2):
            states[r, :, s, 0:3], states[r, :, s, 3:6], states[r, :, s, 6:9] = pos[2 * r + s], vel[2 * r + s], acc[2 * r + s]
    pt = np.array([g["planning_time"][0], g["planning_time"][2]])
    path = tmp_path / "mission_0.csv"
    closed_loop.write_flight_csv(str(path), states, np.zeros((2, 0, 4), np.float32), 0.2, 0.1, pt)
    lines = path.read_text().splitlines()
    assert len(lines) == 5 and lines[:4] == g["raw_lines"]
    obstacles = np.array([[[3, -1, 1, 0.15], [4, -1, 1, 0.3]], [[3.05, -1, 1, 0.15], [4.05, -1, 1, 0.3]]], np.float32)
    closed_loop.write_flight_csv(str(path), states[:, :2], obstacles, 0.2, 0.1)
    lines = [ln.split(",") for ln in path.read_text().splitlines()]
    assert lines[0][24:] == ["obs_id", "t", "px", "py", "pz", "size"] * 2 and all(len(ln) == 36 for ln in lines)
    assert lines[1][24:] == ["0", "0", "3", "-1", "1", "0.15", "1", "0", "4", "-1", "1", "0.3"]
    assert lines[4][24:] == ["0", "0.3", "3.05", "-1", "1", "0.15", "1", "0.3", "4.05", "-1", "1", "0.3"] and lines[4][11] == "0"
