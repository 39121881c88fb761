"""Numpy restatement of the reference's two obstacle classes whose next state depends on more than the time (include/obstacle.hpp):
ChasingObstacle::getChasingObstacle :313-363 and GaussianObstacle::getGaussianObstacle :424-468, driven as ObstacleGenerator::
updateObstacles drives them (include/obstacle_generator.hpp:76-93): every chaser is handed the OTHER obstacles as the previous update left
them, then every obstacle is updated.  Written from the reference's text, not from the library's, in the style of tests/obstacle_reference.py:
float32 wherever the reference works on point3d (positions, velocities, goal points: octomath::Vector3), Python floats (double) everywhere
else -- Python never contracts a multiply and an add.

What is fixed HERE and not by the reference's text:
  * the norm of an Eigen::Vector3d is sqrt((x*x + y*y) + z*z); Eigen's own order depends on its version and vectorisation;
  * ONE update per replan.  MultiSyncSimulator::broadcastMsgs repeats ObstacleGenerator::update once per agent at the same time, i.e.
    with dt = 0 for a chaser; that repetition is not restated;
  * a chaser is a function of the table: its own previous position and velocity are read from its table entry, and its dt is
    t(r) - t(r - 1) of the replan clock r, 0 at r = 0 (t_last_called starts at 0) -- the same figures the reference's member variables hold in a
    flight that is stepped replan by replan;
  * past the end of its acceleration history a gaussian obstacle accelerates by zero (the reference draws ten more seconds there).
Every branch counts itself in `counts`, so that a test can show that its scenario takes each one both ways."""
import collections
import math

import numpy as np

from tests import obstacle_reference as R

f32 = np.float32
SP_EPSILON_FLOAT = 1e-5
DRIVE_NONE, DRIVE_CHASING, DRIVE_GAUSSIAN = 0, 1, 2
HISTORY_ENDED = 1

counts = collections.Counter()


def norm3(v):
    return math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def _p(v):
    return [f32(v[0]), f32(v[1]), f32(v[2])]


class Chasing:
    """The parameters of one ChasingObstacle; `update` is getChasingObstacle with current_state and t_last_called handed in."""

    def __init__(self, radius, max_vel, max_acc, gamma_target, gamma_obs):
        self.radius, self.max_vel, self.max_acc = float(radius), float(max_vel), float(max_acc)
        self.gamma_target, self.gamma_obs = float(gamma_target), float(gamma_obs)

    def update(self, position, velocity, goal_point, obstacles, t, t_last_called):
        """position, velocity, goal_point: point3d; obstacles: [(point3d position, radius)] of the other entries, in table order.
        Returns the new (position, velocity) as float32 lists."""
        position, velocity, goal_point = _p(position), _p(velocity), _p(goal_point)
        delta_goal = [float(goal_point[k] - position[k]) for k in range(3)]  # float differences, widened
        a = [self.gamma_target * d for d in delta_goal]
        v = [float(c) for c in velocity]
        dt = t - t_last_called
        for o_position, o_radius in obstacles:
            o_position = _p(o_position)
            delta_obstacle = [float(o_position[k] - position[k]) for k in range(3)]
            dist_to_obs = norm3(delta_obstacle)
            if dist_to_obs < SP_EPSILON_FLOAT:
                counts["skip"] += 1
                continue
            q_star = 2 * (self.radius + float(o_radius))
            if dist_to_obs < q_star:
                counts["repulsion_inside"] += 1
                s = self.gamma_obs * (1 - dist_to_obs / q_star) * (1 / (dist_to_obs * q_star))
                for k in range(3):
                    a[k] += s * (-(delta_obstacle[k] / dist_to_obs))  # -delta_obstacle.normalized()
            else:
                counts["repulsion_outside"] += 1
        if norm3(a) > (self.max_acc - 0.01):
            counts["acc_clamp_on"] += 1
            na = norm3(a)
            a = [c / na * (self.max_acc - 0.01) for c in a]
        else:
            counts["acc_clamp_off"] += 1
        v = [v[k] + a[k] * dt for k in range(3)]
        if norm3(v) > self.max_vel:
            counts["speed_clamp_on"] += 1
            nv = norm3(v)
            v = [c / nv * self.max_vel for c in v]
        else:
            counts["speed_clamp_off"] += 1
        position = [f32(float(position[k]) + v[k] * dt) for k in range(3)]  # point3d += double
        return position, [f32(c) for c in v]


class Gaussian:
    def __init__(self, start, initial_vel, max_vel, acc_update_cycle, acc_history):
        self.start, self.initial_vel = _p(start), _p(initial_vel)
        self.max_vel, self.acc_update_cycle = float(max_vel), float(acc_update_cycle)
        self.acc_history = [[float(c) for c in a] for a in acc_history]

    def at(self, t):
        """getGaussianObstacle(t): the loop from zero.  Returns (position, velocity, history ended)."""
        position, velocity = list(self.start), list(self.initial_vel)
        n = int(math.floor((t + SP_EPSILON_FLOAT) / self.acc_update_cycle))
        v = [float(c) for c in self.initial_vel]
        dt = self.acc_update_cycle
        ended = False
        for i in range(n + 1):
            if i == n:
                dt = t - n * self.acc_update_cycle
            if i < len(self.acc_history):
                acc = self.acc_history[i]
            else:
                acc, ended = [0.0, 0.0, 0.0], True
            v_next = [v[k] + acc[k] * dt for k in range(3)]
            if norm3(v_next) > self.max_vel:
                counts["gaussian_over"] += 1
                for k in range(3):
                    position[k] = f32(float(position[k]) + v[k] * dt)
            else:
                counts["gaussian_under"] += 1
                for k in range(3):
                    position[k] = f32(float(position[k]) + (v[k] * dt + 0.5 * acc[k] * dt * dt))
                    velocity[k] = f32(float(velocity[k]) + acc[k] * dt)
                v = v_next
        if ended:
            counts["history_ended"] += 1
        return position, velocity, ended


def drive_table(models, drives, acc_history, table, state, r, time_step):
    """One replan of the drives over `table` (api.OBSTACLE_DTYPE, the table as the previous replan left it), in place: what
    ObstacleGenerator::updateObstacles does for the chasing and gaussian entries at clock r.  models: api.OBSTACLE_MODEL_DTYPE (radius,
    max_acc, downwash, start), drives: api.OBSTACLE_DRIVE_DTYPE, acc_history [n_history][3], state [n_total][9] or None.  Entries without a
    drive are not touched."""
    t = R.clock_time(r, time_step)
    t_last = R.clock_time(r - 1, time_step) if r > 0 else 0.0
    prev = [([f32(c) for c in table["position"][i]], float(table["radius"][i])) for i in range(len(table))]
    for i, d in enumerate(drives):
        kind, m = int(d["kind"]), models[i]
        if kind == DRIVE_NONE:
            continue
        ended = False
        if kind == DRIVE_CHASING:
            ta = int(d["target_agent"])
            goal = state[ta][:3] if ta >= 0 else d["goal"]
            c = Chasing(m["radius"], d["max_vel"], m["max_acc"], d["gamma_target"], d["gamma_obs"])
            p, v = c.update(prev[i][0], table["velocity"][i], goal, prev[:i] + prev[i + 1:], t, t_last)
        else:
            first, n = int(d["history_first"]), int(d["history_len"])
            g = Gaussian(m["start"], d["initial_vel"], d["max_vel"], d["acc_update_cycle"], acc_history[first:first + n])
            p, v, ended = g.at(t)
        e = table[i]
        e["position"], e["velocity"] = [float(c) for c in p], [float(c) for c in v]
        e["radius"], e["downwash"], e["max_acc"], e["type"] = m["radius"], m["downwash"], m["max_acc"], 0
        e["reserved"] = HISTORY_ENDED if ended else 0


def advance_table(models, table, r, time_step):
    """The entries lscqp_obstacles_advance_device writes at clock r (tests/obstacle_reference.py), in place."""
    t = R.clock_time(r, time_step)
    for i, m in enumerate(models):
        o = R.from_model(m)
        if o is None:
            continue
        p, v = o.at(t)
        e = table[i]
        e["position"], e["velocity"] = p.astype(np.float64), v.astype(np.float64)
        e["radius"], e["downwash"], e["max_acc"], e["type"], e["reserved"] = o.radius, o.downwash, o.max_acc, 0, 0
