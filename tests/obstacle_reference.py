"""Numpy restatement of the reference's dynamic obstacle models (include/obstacle.hpp): StraightObstacle :138-214, PatrolObstacle
:216-264, SpinObstacle :83-136, and the clock they are evaluated at (src/multi_sync_simulator.cpp:148-153, 311).  Written from the
reference's text, not from the library's: float32 wherever the reference works on point3d (octomath::Vector3, three floats), Python
floats (double) everywhere else, and the patrol finds its leg by the reference's own repeated subtraction from t = 0.

octomath::Vector3: operator+ / - / *(float) per component in float; distance() = double sqrt of the double sum of the squared float
differences; norm() = double sqrt of the FLOAT expression x*x + y*y + z*z; normalized() divides by (float)norm() when it is > 0."""
import math

import numpy as np

f32 = np.float32


def clock_time(r, time_step):
    """(sim_current_time - sim_start_time).toSec() after r steps of `sim_current_time += ros::Duration(time_step)`: a Duration holds whole
    nanoseconds, toSec() is sec + 1e-9 * nsec."""
    ns = int(r) * int(math.floor(time_step * 1e9 + 0.5))
    return float(ns // 10 ** 9) + 1e-9 * float(ns % 10 ** 9)


def _v(p):
    return np.array([f32(p[0]), f32(p[1]), f32(p[2])], dtype=f32)


def _mul(v, k):  # Vector3::operator*(float): the factor is narrowed first
    return (v * f32(k)).astype(f32)


class Straight:
    def __init__(self, start, goal, radius, speed, max_acc, downwash):
        self.radius, self.speed, self.max_acc, self.downwash = float(radius), float(speed), float(max_acc), float(downwash)
        self.start, self.goal = _v(start), _v(goal)
        d = [float(self.start[k] - self.goal[k]) for k in range(3)]  # float differences, widened
        self.dist_to_goal = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        self.dist_acc = 0.5 * self.speed * self.speed / self.max_acc
        g = (self.goal - self.start).astype(f32)
        norm = math.sqrt(float(f32(f32(g[0] * g[0]) + f32(g[1] * g[1])) + f32(g[2] * g[2])))
        self.n = (g / f32(norm)).astype(f32) if norm > 0 else g
        if self.dist_to_goal > 2 * self.dist_acc:
            self.flight_time = (self.dist_to_goal - 2 * self.dist_acc) / self.speed + 2 * self.speed / self.max_acc
        else:
            self.flight_time = 2 * math.sqrt(self.dist_to_goal / self.dist_acc)

    def phases(self):
        """The phase boundaries (t1, t2, t3) of the long branch, (t1, t2) of the short one."""
        if self.dist_to_goal > 2 * self.dist_acc:
            t1 = self.speed / self.max_acc
            t2 = t1 + (self.dist_to_goal - 2 * self.dist_acc) / self.speed
            return (t1, t2, t1 + t2)
        t1 = math.sqrt(self.dist_to_goal / self.dist_acc)
        return (t1, 2 * t1)

    def _half_acc(self, u):  # n * 0.5 * max_acc * u * u, left to right
        return _mul(_mul(_mul(_mul(self.n, 0.5), self.max_acc), u), u)

    def at(self, t):
        """(position, velocity) as float32 vectors."""
        n, s, g, a, v = self.n, self.start, self.goal, self.max_acc, self.speed
        pos, vel = g.copy(), np.zeros(3, f32)
        if self.dist_to_goal > 2 * self.dist_acc:
            t1, t2, t3 = self.phases()
            if t < t1:
                pos, vel = s + self._half_acc(t), _mul(_mul(n, a), t)
            elif t < t2:
                pos, vel = s + _mul(n, 0.5 * a * t1 * t1 + v * (t - t1)), _mul(n, v)
            elif t < t3:
                pos, vel = g - self._half_acc(t3 - t), _mul(n, v - a * (t - t2))
        else:
            t1, t2 = self.phases()
            if t < t1:
                pos, vel = s + self._half_acc(t), _mul(_mul(n, a), t)
            elif t < t2:
                pos, vel = g - self._half_acc(t2 - t), _mul(_mul(n, a), t2 - t)
        return pos.astype(f32), vel.astype(f32)


class Patrol:
    def __init__(self, waypoints, radius, speed, max_acc, downwash):
        self.radius, self.speed, self.max_acc, self.downwash = float(radius), float(speed), float(max_acc), float(downwash)
        w = [list(p) for p in waypoints]
        self.legs = [Straight(w[i], w[(i + 1) % len(w)], radius, speed, max_acc, downwash) for i in range(len(w))]
        self.flight_time = [leg.flight_time for leg in self.legs]

    def lap_time(self):
        lap = 0.0
        for ft in self.flight_time:
            lap += ft
        return lap

    def at(self, t):
        cur, idx = t, 0
        while cur >= self.flight_time[idx]:  # the reference's search: every leg of every lap since t = 0
            cur -= self.flight_time[idx]
            idx = 0 if idx == len(self.legs) - 1 else idx + 1
        return self.legs[idx].at(cur)


def _qmul(a, b):
    return (a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1])


def _qinv(a):
    n2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + a[3] * a[3]
    return (a[0] / n2, -a[1] / n2, -a[2] / n2, -a[3] / n2)


class Spin:
    def __init__(self, axis_point, axis_direction, start, radius, speed, max_acc, downwash):
        self.radius, self.speed, self.max_acc, self.downwash = float(radius), float(speed), float(max_acc), float(downwash)
        self.axis_point = [float(c) for c in axis_point]
        d = [float(c) for c in axis_direction]
        ln = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        self.n = [c / ln for c in d]
        self.a = [float(start[k]) - self.axis_point[k] for k in range(3)]
        dot = self.a[0] * self.n[0] + self.a[1] * self.n[1] + self.a[2] * self.n[2]
        r = [self.a[k] - dot * self.n[k] for k in range(3)]
        self.spin_radius = math.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
        self.w = self.speed / self.spin_radius

    def at(self, t):
        n, theta = self.n, self.w * t
        q = (math.cos(theta / 2), math.sin(theta / 2) * n[0], math.sin(theta / 2) * n[1], math.sin(theta / 2) * n[2])
        p = _qmul(_qmul(q, (0.0, self.a[0], self.a[1], self.a[2])), _qinv(q))
        pos = np.array([f32(self.axis_point[k] + p[1 + k]) for k in range(3)], f32)
        theta = math.pi / 2
        qv = (math.cos(theta / 2), math.sin(theta / 2) * n[0], math.sin(theta / 2) * n[1], math.sin(theta / 2) * n[2])
        p = _qmul(_qmul(qv, p), _qinv(qv))
        vel = np.array([f32(self.w * p[1 + k]) for k in range(3)], f32)
        return pos, vel


def from_model(m):
    """The restatement's object for one api.OBSTACLE_MODEL_DTYPE record (its input fields only); None for a HELD model."""
    kind = int(m["kind"])
    common = (float(m["radius"]), float(m["speed"]), float(m["max_acc"]), float(m["downwash"]))
    if kind == 1:
        return Straight(m["start"], m["goal"], *common)
    if kind == 2:
        return Patrol(m["waypoints"][:int(m["n_waypoints"])], *common)
    if kind == 3:
        return Spin(m["axis_point"], m["axis_direction"], m["start"], *common)
    return None


def table_at(models, r, time_step):
    """position, velocity [n][3] as float32 of every model at replan r (HELD rows: NaN)."""
    t = clock_time(r, time_step)
    pos, vel = np.full((len(models), 3), np.nan, f32), np.full((len(models), 3), np.nan, f32)
    for i, m in enumerate(models):
        o = from_model(m)
        if o is not None:
            pos[i], vel[i] = o.at(t)
    return pos, vel
