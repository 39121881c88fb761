"""The flight log (include/lscqp.h, "the flight log"; csrc/lscrecord.hip: flight_log_kernel) in numpy: the sampled state of a plan in
float64 from its float32 control points (csrc/lscpost_traj.hpp: state_at), the index functions of the log's layout, and the flags word."""
from math import comb

import numpy as np

FLAG_QP_FAILED, FLAG_INVALID, FLAG_GOAL_FAILED, FLAG_SFC_KEPT, FLAG_WAYPOINT = 1, 2, 4, 8, 16
FLAG_FIELDS = ("qp_failed", "invalid", "goal_failed", "sfc_kept", "waypoint_updates")  # the record's counter of bit i
STATUS_OPTIMAL = 0


def segment_of(t, M, dt):
    """getPointAt's segment search (src/trajectory.cpp:121-136): (segment, normalised time); beyond the horizon the last segment at 1."""
    end = 0.0
    for idx in range(M):
        end += dt
        if t < end:
            return idx, 1 - (end - t) / dt
    return M - 1, 1.0


def _bern(n, tn):
    return np.array([comb(n, i) * tn ** i * (1 - tn) ** (n - i) for i in range(n + 1)])


def states_f64(x, M, dim, dt, n_samples, record_time_step, z_2d):
    """(n, S, 9) float64: position, velocity and acceleration of the plans x (n, dim*M*6) at s * record_time_step.  Control points
    narrowed to float32, derivative control points d1[i] = (c[i+1] - c[i]) * (5/dt) and d2[i] = (d1[i+1] - d1[i]) * (4/dt), the three
    Bernstein sums, all in float64.  Axes k >= dim: position float32(z_2d), velocity and acceleration 0."""
    c = np.asarray(x, np.float64).reshape(-1, dim, M, 6).astype(np.float32).astype(np.float64)
    out = np.zeros((c.shape[0], n_samples, 9))
    for s in range(n_samples):
        ms, tn = segment_of(s * record_time_step, M, dt)
        cs = c[:, :, ms, :]
        d1 = (cs[..., 1:] - cs[..., :-1]) * (5.0 / dt)
        d2 = (d1[..., 1:] - d1[..., :-1]) * (4.0 / dt)
        out[:, s, 0:dim] = cs @ _bern(5, tn)
        out[:, s, 3:3 + dim] = d1 @ _bern(4, tn)
        out[:, s, 6:6 + dim] = d2 @ _bern(3, tn)
        if dim < 3:
            out[:, s, dim:3] = float(np.float32(z_2d))
    return out


def flags_word(status, valid, goal_status, sfc_status, waypoint_updated=None):
    """int32 (n,): bit 0 QP status != OPTIMAL, bit 1 valid == 0, bit 2 goal LP status != 0, bit 3 sfc_status == 0, bit 4 waypoint updated."""
    w = (np.asarray(status) != STATUS_OPTIMAL) * FLAG_QP_FAILED + (np.asarray(valid) == 0) * FLAG_INVALID
    w = w + (np.asarray(goal_status) != 0) * FLAG_GOAL_FAILED + (np.asarray(sfc_status) == 0) * FLAG_SFC_KEPT
    if waypoint_updated is not None:
        w = w + (np.asarray(waypoint_updated) != 0) * FLAG_WAYPOINT
    return w.astype(np.int32)


# ---- the layout: off[] the partition, n_k = off[k+1] - off[k], S samples, C = max_replans, every index in ELEMENTS of its buffer ----------
def state_block(off, k, S, C):
    """[first, end) of mission k's block in the states buffer (floats)."""
    return C * int(off[k]) * S * 9, C * int(off[k + 1]) * S * 9


def state_index(off, k, r, a, s, S, C):
    """Index of px of (mission k, replan r, GLOBAL agent a, sample s); the nine floats follow one another."""
    n_k = int(off[k + 1]) - int(off[k])
    return C * int(off[k]) * S * 9 + ((r * n_k + (a - int(off[k]))) * S + s) * 9


def flag_block(off, k, C):
    return C * int(off[k]), C * int(off[k + 1])


def flag_index(off, k, r, a, C):
    n_k = int(off[k + 1]) - int(off[k])
    return C * int(off[k]) + r * n_k + (a - int(off[k]))


def obstacle_index(k, r, oi, n_dyn, C):
    """Index of px of (mission k, replan r, obstacle oi); px, py, pz, radius follow one another."""
    return ((k * C + r) * n_dyn + oi) * 4


def sizes(off, S, C, n_dyn):
    """Elements of the three buffers: states (float32), flags (int32), obstacles (float32)."""
    n, K = int(off[-1]), len(off) - 1
    return C * n * S * 9, C * n, K * C * n_dyn * 4


def mission_views(off, k, S, C, n_dyn, states, flags, obstacles):
    """One mission's blocks of the three raw buffers as (C, n_k, S, 9), (C, n_k) and (C, n_dyn, 4) views."""
    n_k = int(off[k + 1]) - int(off[k])
    a, b = state_block(off, k, S, C)
    fa, fb = flag_block(off, k, C)
    o = obstacle_index(k, 0, 0, n_dyn, C)
    return (states[a:b].reshape(C, n_k, S, 9), flags[fa:fb].reshape(C, n_k), obstacles[o:o + C * n_dyn * 4].reshape(C, n_dyn, 4))
