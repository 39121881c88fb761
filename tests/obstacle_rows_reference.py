"""Numpy restatement of TrajPlanner::generateCLSC for a NON-AGENT obstacle -- TEST INFRASTRUCTURE.

Written from the reference's text: src/traj_planner.cpp:659-706 (generateCLSC), :1179-1205 (normalVectorBetweenPolys), :1229-1240
(downwashBetween) and src/trajectory.cpp:79-91 (planConstVelTraj); float32 wherever the reference works on point3d (octomath::Vector3),
Python floats (double) elsewhere.  Two pieces are borrowed, as arbiters and not as copies of the code under test: the closest point of
the relative hull comes from the exact referee (tests/hull_reference.py, rational arithmetic) and the closest points of the last
segment's two line segments from oracle.segseg_closest (held to an exact fixture by tests/test_lscmode.py).

octomath::Vector3: operator+ / - / *(float) per component in float; dot() the float expression x x' + y y' + z z' widened to double;
norm() the double sqrt of the float expression x x + y y + z z; normalized() divides by (float)norm() when it is > 0."""
import math

import numpy as np

f32 = np.float32


def _v(p):
    return np.array([f32(p[0]), f32(p[1]), f32(p[2])], dtype=f32)


def _dot(a, b):
    return float(f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2])))


def _normalized(a):
    ln = math.sqrt(_dot(a, a))
    return (a / f32(ln)).astype(f32) if ln > 0 else a.copy()


def predicted_points(M, dt, position, velocity):
    """planConstVelTraj: control point (m, i) = position + velocity * (float)time, `time` a double that advances by dt / 5 after EVERY
    control point (six steps per segment, the reference's own quirk).  (M, 6, 3) float32."""
    p, v = _v(position), _v(velocity)
    out = np.zeros((M, 6, 3), f32)
    time = 0.0
    for m in range(M):
        for i in range(6):
            out[m, i] = p + (v * f32(time)).astype(f32)
            time += dt / 5
    return out


def downwash_between(r_own, ob):
    """:1235-1237, the non-agent branch"""
    return (r_own + float(ob["downwash"]) * float(ob["radius"])) / (r_own + float(ob["radius"]))


def is_tall(ob, obs_downwash_threshold):
    return int(ob["type"]) == 0 and float(ob["downwash"]) > obs_downwash_threshold


def _trf(p, dw, dim):
    q = _v(p)
    if dim != 2:  # generateCLSC transforms in 3-D only (:666-672); Trajectory::coordinateTransform divides z by (float)downwash
        q[2] = q[2] / f32(dw)
    return q


def clsc_obstacle_rows(oracle, referee, M, dim, dt, own, agent_goal, r_own, ob, obs_downwash_threshold=3.0, obstacle_goal=None, records=False):
    """Rows (nx, ny, nz, b)[M][6] of one (agent, obstacle) pair: own (M, 6, 3) the agent's initial trajectory, ob a record with position,
    velocity, radius, downwash, type; obstacle_goal None = point3d's default, the origin.
    The row is what TrajOptimizer::populatebyrow makes of the LSC record (obs_control_point p, normal_vector n, d): sum over k < dim of
    n_k (x_k - p_k) >= d (src/traj_optimizer.cpp:414-421), i.e. b = d + n_x p_x + n_y p_y and n_z = 0 in 2-D whatever z the record's
    normal has -- on the last segment it has one when the obstacle's goal point lies off the mission's plane.
    records=True: also the records themselves, (p (M, 6, 3), n (M, 3) as setLSC gets it, d (M, 6))."""
    own = np.asarray(own, dtype=np.float64)
    pred = predicted_points(M, dt, ob["position"], ob["velocity"])
    collision_dist = float(ob["radius"]) + r_own
    dw = downwash_between(r_own, ob)
    tall = is_tall(ob, obs_downwash_threshold)
    out = np.zeros((M, 6, 4))
    rec_p, rec_n, rec_d = np.zeros((M, 6, 3)), np.zeros((M, 3)), np.zeros((M, 6))
    for m in range(M):
        if m < M - 1:
            rel = np.array([(_trf(own[m, i], dw, dim) - _trf(pred[m, i], dw, dim)).astype(f32) for i in range(6)], dtype=f32)
            hull = rel.astype(np.float64)
            if tall:
                hull[:, 2] = 0.0
            r = referee.closest_point(hull)
            if r.inside:
                n = np.zeros(3, f32)
            else:
                n = _normalized(np.array([float(x) for x in r.point]).astype(f32))
            d = [0.5 * (collision_dist + _dot(rel[i], n)) for i in range(6)]
            p_obs = pred[m].astype(np.float64)
        else:
            go = np.zeros(3) if obstacle_goal is None else np.asarray(obstacle_goal, dtype=np.float64)
            dist, c1, c2 = oracle.segseg_closest(_trf(pred[M - 1, 5], dw, dim), _v(go), _trf(own[M - 1, 5], dw, dim), _v(agent_goal))
            n = _normalized((_v(c2) - _v(c1)).astype(f32))
            d = [0.5 * (collision_dist + dist)] * 6
            p_obs = np.tile(np.asarray(c1, dtype=np.float64), (6, 1))
        n_rec = np.array([float(n[0]), float(n[1]), float(f32(float(n[2]) / dw))])  # normal_vector.z() / downwash, then setLSC
        rec_p[m], rec_n[m], rec_d[m] = p_obs, n_rec, d
        n_out = n_rec * np.array([1.0, 1.0, 1.0 if dim == 3 else 0.0])
        out[m, :, :3] = n_out
        out[m, :, 3] = np.array(d) + p_obs @ n_out
    return (out, (rec_p, rec_n, rec_d)) if records else out
