"""The mission record (include/lscqp.h, "the mission record") restated in numpy from the reference's source, float32 where the reference
computes in float32:
    MultiSyncSimulator::isFinished        src/multi_sync_simulator.cpp:401-424   (point3d::distance against param.goal_threshold)
    MultiSyncSimulator::getTotalDistance  :711-720                               (norm() of consecutive logged points, summed in double)
    MultiSyncSimulator::update            :486-577                               (minimum safety ratio, maximum excess ratios)
The sample points themselves are an INPUT here (the device's points buffer, or a log): Trajectory::getStateAt is restated elsewhere
(oracle.state_at), and `points_f64` below evaluates it in float64 for the one bound the GPU tests put on the device's points."""
from math import comb

import numpy as np

SAFETY_DTYPE = np.dtype([("safety_ratio", "f8"), ("closest_agent", "i4"), ("sample", "i4"), ("vel_excess_ratio", "f8", 3), ("acc_excess_ratio", "f8", 3)])
FIELDS = ("finished", "replans", "first_qp_failed_replan", "flight_time", "distance", "safety_ratio_agent", "safety_replan", "safety_agent", "safety_other",
          "vel_excess_ratio", "acc_excess_ratio", "qp_failed", "invalid", "goal_failed", "sfc_kept", "waypoint_updates", "max_in_range", "truncated")


def vector3_norm(d):
    """octomath::Vector3::norm of float32 rows d (n, 3): float sum of squares, its square root in double."""
    d = np.asarray(d, np.float32)
    nsq = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]  # float32 throughout, left to right
    assert nsq.dtype == np.float32
    return np.sqrt(nsq.astype(np.float64))


def vector3_distance(a, b):
    """Vector3::distance = (a - b).norm() on float32 values."""
    return vector3_norm(np.asarray(a, np.float32) - np.asarray(b, np.float32))


def neutral_safety(n):
    s = np.zeros(n, SAFETY_DTYPE)
    s["safety_ratio"], s["closest_agent"], s["sample"] = np.inf, -1, -1
    return s


class Record:
    def __init__(self, n_total, goal_points, goal_threshold, time_step, offsets=None):
        self.n = int(n_total)
        self.off = np.array([0, self.n] if offsets is None else offsets, dtype=np.int64)
        self.K = len(self.off) - 1
        self.thr, self.time_step = float(goal_threshold), float(time_step)
        self.reset(goal_points)

    def reset(self, goal_points):
        self.goal = np.asarray(goal_points, np.float64).reshape(self.n, 3).astype(np.float32)
        self.dist = np.zeros(self.n, np.float64)
        self.last = np.zeros((self.n, 3), np.float32)
        self.unfinished = self.K
        self.m = [dict(finished=0, replans=0, first_qp_failed_replan=-1, flight_time=-1.0, safety_ratio_agent=np.inf, safety_replan=-1, safety_agent=-1,
                       safety_other=-1, vel_excess_ratio=np.zeros(3), acc_excess_ratio=np.zeros(3), qp_failed=0, invalid=0, goal_failed=0, sfc_kept=0,
                       waypoint_updates=0, max_in_range=0, truncated=0) for _ in range(self.K)]

    def step(self, points, p0, status, goal_status, sfc_status, valid, in_range, n_obs, safety, waypoint_updated=None):
        """One replan: points (n, S, 3) float32 of the NEW plans, p0 (n, 3) the positions the replan started from, the chain's int32 buffers,
        n_obs (n,) the headers' row slots, safety (n,) SAFETY_DTYPE."""
        points = np.asarray(points, np.float32).reshape(self.n, -1, 3)
        p0 = np.asarray(p0, np.float64).reshape(self.n, 3).astype(np.float32)
        n_obs = np.broadcast_to(np.asarray(n_obs), (self.n,))
        for k, m in enumerate(self.m):
            if m["finished"]:
                continue  # frozen
            r = m["replans"]
            lo, hi = int(self.off[k]), int(self.off[k + 1])
            for a in range(lo, hi):  # the polyline, the segment from the previous replan's last point included (none at r = 0)
                line = points[a] if r == 0 else np.concatenate([self.last[a:a + 1], points[a]])
                for seg in vector3_norm(line[1:] - line[:-1]):
                    self.dist[a] += seg
                self.last[a] = points[a, -1]
            sl = slice(lo, hi)
            ratio = np.asarray(safety["safety_ratio"][sl], np.float64)
            i = int(np.argmin(ratio))  # the first minimum: the lowest agent id
            if ratio[i] < m["safety_ratio_agent"]:  # strict <: the earlier replan keeps a tie
                m["safety_ratio_agent"], m["safety_replan"], m["safety_agent"], m["safety_other"] = float(ratio[i]), r, lo + i, int(safety["closest_agent"][lo + i])
            m["vel_excess_ratio"] = np.maximum(m["vel_excess_ratio"], np.asarray(safety["vel_excess_ratio"][sl], np.float64).max(axis=0))
            m["acc_excess_ratio"] = np.maximum(m["acc_excess_ratio"], np.asarray(safety["acc_excess_ratio"][sl], np.float64).max(axis=0))
            failed = int((np.asarray(status[sl]) != 0).sum())
            m["qp_failed"] += failed
            if failed and m["first_qp_failed_replan"] < 0:
                m["first_qp_failed_replan"] = r
            m["invalid"] += int((np.asarray(valid[sl]) == 0).sum())
            m["goal_failed"] += int((np.asarray(goal_status[sl]) != 0).sum())
            m["sfc_kept"] += int((np.asarray(sfc_status[sl]) == 0).sum())
            if waypoint_updated is not None:
                m["waypoint_updates"] += int((np.asarray(waypoint_updated[sl]) != 0).sum())
            m["max_in_range"] = max(m["max_in_range"], int(np.asarray(in_range[sl]).max()))
            m["truncated"] += int((np.asarray(in_range[sl]) > n_obs[sl]).sum())
            m["replans"] = r + 1
            # isFinished, on the state this replan started from: no agent further than the threshold (compared in double)
            if not (vector3_distance(p0[sl], self.goal[sl]) > self.thr).any():
                m["finished"], m["flight_time"] = 1, r * self.time_step
                self.unfinished -= 1

    def records(self):
        out = []
        for k, m in enumerate(self.m):
            d = dict(m)
            s = 0.0
            for v in self.dist[int(self.off[k]):int(self.off[k + 1])]:  # id order, one addition at a time
                s += float(v)
            d["distance"] = s
            out.append(d)
        return out


def same_records(got, want):
    """Names of the fields in which a downloaded record array (api.MISSION_RECORD_DTYPE) differs from Record.records(): exact comparison."""
    bad = []
    for k, w in enumerate(want):
        for f in FIELDS:
            g = got[f][k]
            if not np.array_equal(np.asarray(g, np.float64), np.asarray(w[f], np.float64)):
                bad.append((k, f, np.asarray(g).tolist(), np.asarray(w[f]).tolist()))
    return bad


def points_f64(x, M, dim, dt, n_samples, record_time_step, z_2d):
    """Trajectory::getStateAt's positions of the float32 control points of plans x (n, dim*M*6) at s * record_time_step, evaluated in
    float64 (getPointAt's segment search, src/trajectory.cpp:121-136, and the Bernstein sum): (n, S, 3) float64."""
    x = np.asarray(x, np.float64).reshape(-1, dim, M, 6).astype(np.float32).astype(np.float64)
    out = np.zeros((x.shape[0], n_samples, 3))
    for s in range(n_samples):
        t = s * record_time_step
        ms, tn, end = M - 1, 1.0, 0.0
        for idx in range(M):
            end += dt
            if t < end:
                ms, tn = idx, 1 - (end - t) / dt
                break
        b = np.array([comb(5, i) * tn ** i * (1 - tn) ** (5 - i) for i in range(6)])
        out[:, s, :dim] = x[:, :, ms, :] @ b
        if dim < 3:
            out[:, s, dim:] = float(np.float32(z_2d))
    return out
