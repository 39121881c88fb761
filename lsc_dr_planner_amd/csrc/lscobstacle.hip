// lscobstacle.hip — how the mission's dynamic obstacles move, on the device, gfx950 only: the device analogue of
//   ObstacleGenerator::update(t, 0)      reference include/obstacle_generator.hpp:28-35, 95-110 (no observer noise)
//   StraightObstacle / PatrolObstacle / SpinObstacle::getObstacle   include/obstacle.hpp:83-264
// One kernel moves the whole obstacle table of a plan by one replan; lscplan.hip puts it in front of its chain.  The per-leg
// constants of StraightObstacle's constructor are made once on the host (lscqp_obstacle_model_prepare: no device needed), in the
// reference's own arithmetic: point3d is octomath::Vector3, three FLOATS -- Vector3::distance is the double square root of the double
// sum of squared float differences, normalized() divides by (float)norm(), norm() is the double square root of a float sum of squares,
// and `n * 0.5 * max_acc * t * t` is four Vector3::operator*(float) in a row.  Nothing here may contract a multiply and an add.
// This file has no object of its own: lscplan.hip includes it (as lscsfc_tp.hip includes lscsfc.hip), so that it is built with
// the chain that launches its kernel.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/lscqp.h"
#include "lscqp_internal.hpp"

namespace lscobstacle {

constexpr int kThreads = 64;

struct F3 {
    float x, y, z;
};

// StraightObstacle::getStraightObstacle (include/obstacle.hpp:175-213) of one leg at leg time t.  vel stays the zero vector where the
// reference leaves obs_velocity default-constructed (past the last phase).
__host__ __device__ inline void straight_at(const lscqp_obstacle_leg& L, double speed, double max_acc, double t, F3* pos, F3* vel) {
#pragma clang fp contract(off)
    const F3 s{L.start[0], L.start[1], L.start[2]}, g{L.goal[0], L.goal[1], L.goal[2]}, n{L.n[0], L.n[1], L.n[2]};
    auto mul = [](F3 a, float k) { return F3{a.x * k, a.y * k, a.z * k}; };
    auto add = [](F3 a, F3 b) { return F3{a.x + b.x, a.y + b.y, a.z + b.z}; };
    auto sub = [](F3 a, F3 b) { return F3{a.x - b.x, a.y - b.y, a.z - b.z}; };
    // n * 0.5 * max_acc * u * u: left to right, every factor narrowed to float by Vector3::operator*(float)
    auto half_acc = [&](double u) { return mul(mul(mul(mul(n, 0.5f), (float)max_acc), (float)u), (float)u); };
    F3 p = g, v{0.0f, 0.0f, 0.0f};
    if (L.dist_to_goal > 2 * L.dist_acc) {
        const double t1 = speed / max_acc;
        const double t2 = t1 + (L.dist_to_goal - 2 * L.dist_acc) / speed;
        const double t3 = t1 + t2;
        if (t < t1) {
            p = add(s, half_acc(t));
            v = mul(mul(n, (float)max_acc), (float)t);
        } else if (t < t2) {
            p = add(s, mul(n, (float)(0.5 * max_acc * t1 * t1 + speed * (t - t1))));
            v = mul(n, (float)speed);
        } else if (t < t3) {
            p = sub(g, half_acc(t3 - t));
            v = mul(n, (float)(speed - max_acc * (t - t2)));
        }
    } else {
        const double t1 = sqrt(L.dist_to_goal / L.dist_acc);
        const double t2 = 2 * t1;
        if (t < t1) {
            p = add(s, half_acc(t));
            v = mul(mul(n, (float)max_acc), (float)t);
        } else if (t < t2) {
            p = sub(g, half_acc(t2 - t));
            v = mul(mul(n, (float)max_acc), (float)(t2 - t));
        }
    }
    *pos = p;
    *vel = v;
}

// PatrolObstacle::getPatrolObstacle (:246-263) in O(legs): whole laps off first, then at most n_legs legs
__host__ __device__ inline void patrol_at(const lscqp_obstacle_model& m, double t, F3* pos, F3* vel) {
#pragma clang fp contract(off)
    double cur = t;
    if (cur >= m.lap_time) {
        cur = t - floor(t / m.lap_time) * m.lap_time;
        if (cur < 0) cur += m.lap_time;  // (the quotient rounded up across a whole number)
    }
    // (a model that was not prepared must not index past its legs)
    const int n_legs = m.n_legs < 1 ? 1 : (m.n_legs > LSCQP_OBSTACLE_MAX_WAYPOINTS ? LSCQP_OBSTACLE_MAX_WAYPOINTS : m.n_legs);
    int idx = 0;
    for (int i = 0; i < n_legs; i++) {
        if (!(cur >= m.leg[idx].flight_time)) break;
        cur -= m.leg[idx].flight_time;
        idx = (idx == n_legs - 1) ? 0 : idx + 1;
    }
    straight_at(m.leg[idx], m.speed, m.max_acc, cur, pos, vel);
}

// SpinObstacle::getSpinObstacle (:100-135): p = q (0, a) q^-1 with q = (cos th/2, sin th/2 n), then the same with th = pi/2 for the velocity
__host__ __device__ inline void spin_at(const lscqp_obstacle_model& m, double t, F3* pos, F3* vel) {
#pragma clang fp contract(off)
    struct Q {
        double w, x, y, z;
    };
    auto prod = [](Q a, Q b) {
        return Q{a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
                 a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z, a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x};
    };
    auto inverse = [](Q a) {
        const double n2 = a.w * a.w + a.x * a.x + a.y * a.y + a.z * a.z;
        return Q{a.w / n2, -a.x / n2, -a.y / n2, -a.z / n2};
    };
    const double* n = m.spin_axis;
    const double theta = m.spin_w * t;
    const double c = cos(theta / 2), s = sin(theta / 2);
    const Q q{c, s * n[0], s * n[1], s * n[2]};
    Q p{0.0, m.spin_offset[0], m.spin_offset[1], m.spin_offset[2]};
    p = prod(prod(q, p), inverse(q));
    *pos = F3{(float)(m.axis_point[0] + p.x), (float)(m.axis_point[1] + p.y), (float)(m.axis_point[2] + p.z)};
    const double half = 3.14159265358979323846 / 2 / 2;  // M_PI / 2, halved
    const double cv = cos(half), sv = sin(half);
    const Q qv{cv, sv * n[0], sv * n[1], sv * n[2]};
    p = prod(prod(qv, p), inverse(qv));
    *vel = F3{(float)(m.spin_w * p.x), (float)(m.spin_w * p.y), (float)(m.spin_w * p.z)};
}

// One workgroup; thread i takes obstacles i, i + 64, ...  The clock word is read by every thread before the barrier and written by
// thread 0 behind it.  t: r steps of ros::Duration(time_step) -- step_ns whole nanoseconds each -- then Duration::toSec().
__global__ __launch_bounds__(kThreads) void obstacle_advance_kernel(const lscqp_obstacle_model* __restrict__ models, int n_dyn, int64_t step_ns,
                                                                     int32_t* clock, lscqp_obstacle* __restrict__ table) {
#pragma clang fp contract(off)
    const int32_t r = *clock;
    const int64_t ns = (int64_t)r * step_ns;
    const double t = (double)(ns / 1000000000LL) + 1e-9 * (double)(ns % 1000000000LL);
    for (int oi = threadIdx.x; oi < n_dyn; oi += kThreads) {
        const lscqp_obstacle_model& m = models[oi];
        if (m.kind == LSCQP_OBSTACLE_HELD) continue;
        F3 p, v;
        if (m.kind == LSCQP_OBSTACLE_STRAIGHT) straight_at(m.leg[0], m.speed, m.max_acc, t, &p, &v);
        else if (m.kind == LSCQP_OBSTACLE_PATROL) patrol_at(m, t, &p, &v);
        else spin_at(m, t, &p, &v);
        lscqp_obstacle* o = table + oi;
        o->position[0] = (double)p.x, o->position[1] = (double)p.y, o->position[2] = (double)p.z;
        o->velocity[0] = (double)v.x, o->velocity[1] = (double)v.y, o->velocity[2] = (double)v.z;
        o->radius = m.radius, o->downwash = m.downwash, o->max_acc = m.max_acc;
        o->type = 0;  // DYNAMICOBSTACLE (ObstacleBase::getObstacle)
        o->reserved = 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) *clock = r + 1;
}

// StraightObstacle's constructor (:145-161)
inline void make_leg(const double* start, const double* goal, double speed, double max_acc, lscqp_obstacle_leg* L) {
#pragma clang fp contract(off)
    memset(L, 0, sizeof *L);
    float d[3];
    for (int k = 0; k < 3; k++) {
        L->start[k] = (float)start[k];  // pointMsgToPoint3d
        L->goal[k] = (float)goal[k];
    }
    // start.distance(goal): float differences widened, double sum of squares
    const double dx = (double)(L->start[0] - L->goal[0]), dy = (double)(L->start[1] - L->goal[1]), dz = (double)(L->start[2] - L->goal[2]);
    L->dist_to_goal = sqrt(dx * dx + dy * dy + dz * dz);
    L->dist_acc = 0.5 * speed * speed / max_acc;
    // (goal - start).normalized(): float differences, norm() = sqrt of the float sum of squares, divided by (float)norm() if > 0
    for (int k = 0; k < 3; k++) d[k] = L->goal[k] - L->start[k];
    const double len = sqrt((double)(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]));
    for (int k = 0; k < 3; k++) L->n[k] = len > 0 ? d[k] / (float)len : d[k];
    if (L->dist_to_goal > 2 * L->dist_acc) L->flight_time = (L->dist_to_goal - 2 * L->dist_acc) / speed + 2 * speed / max_acc;
    else L->flight_time = 2 * sqrt(L->dist_to_goal / L->dist_acc);
}

inline int refuse(int i, const char* what) {
    char msg[200];
    snprintf(msg, sizeof msg, "lscqp_obstacle_model_prepare: model %d: %s", i, what);
    return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, msg);
}

inline bool finite3(const double* v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }

}  // namespace lscobstacle

extern "C" int lscqp_obstacle_model_prepare(lscqp_obstacle_model* models, int32_t n) {
#pragma clang fp contract(off)
    using namespace lscobstacle;
    if (n < 0) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "negative size");
    if (n == 0) return LSCQP_OK;
    if (!models) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null buffer");
    for (int i = 0; i < n; i++) {
        lscqp_obstacle_model* m = models + i;
        if (m->kind != LSCQP_OBSTACLE_HELD && m->kind != LSCQP_OBSTACLE_STRAIGHT && m->kind != LSCQP_OBSTACLE_PATROL && m->kind != LSCQP_OBSTACLE_SPIN)
            return refuse(i, "kind must be LSCQP_OBSTACLE_HELD, _STRAIGHT, _PATROL or _SPIN");
        if (!isfinite(m->radius) || !isfinite(m->downwash) || !isfinite(m->max_acc) || !isfinite(m->speed) || !finite3(m->start))
            return refuse(i, "a field is not finite (radius, downwash, max_acc, speed, start)");
        if (m->radius < 0) return refuse(i, "radius < 0");
        if (!(m->max_acc > 0)) return refuse(i, "max_acc <= 0");
        m->n_legs = 0, m->lap_time = 0, m->spin_w = 0;
        memset(m->leg, 0, sizeof m->leg);
        memset(m->spin_axis, 0, sizeof m->spin_axis);
        memset(m->spin_offset, 0, sizeof m->spin_offset);
        if (m->kind != LSCQP_OBSTACLE_HELD && !(m->speed > 0)) return refuse(i, "speed <= 0");
        if (m->kind == LSCQP_OBSTACLE_STRAIGHT) {
            if (!finite3(m->goal)) return refuse(i, "a field is not finite (goal)");
            make_leg(m->start, m->goal, m->speed, m->max_acc, &m->leg[0]);
            m->n_legs = 1;
            m->lap_time = m->leg[0].flight_time;
        } else if (m->kind == LSCQP_OBSTACLE_PATROL) {
            if (m->n_waypoints < 1 || m->n_waypoints > LSCQP_OBSTACLE_MAX_WAYPOINTS)
                return refuse(i, "a patrol takes 1 .. LSCQP_OBSTACLE_MAX_WAYPOINTS (8) waypoints");
            for (int w = 0; w < m->n_waypoints; w++)
                if (!finite3(m->waypoints[w])) return refuse(i, "a field is not finite (waypoints)");
            double lap = 0;
            for (int w = 0; w < m->n_waypoints; w++) {
                make_leg(m->waypoints[w], m->waypoints[w + 1 < m->n_waypoints ? w + 1 : 0], m->speed, m->max_acc, &m->leg[w]);
                lap += m->leg[w].flight_time;
            }
            if (!(lap > 0) || !isfinite(lap)) return refuse(i, "the patrol's lap time is not positive (its waypoints coincide)");
            m->n_legs = m->n_waypoints;
            m->lap_time = lap;
        } else if (m->kind == LSCQP_OBSTACLE_SPIN) {
            if (!finite3(m->axis_point) || !finite3(m->axis_direction)) return refuse(i, "a field is not finite (axis_point, axis_direction)");
            const double* d = m->axis_direction;
            const double z = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
            if (!(z > 0)) return refuse(i, "the spin's axis direction is zero");
            double nn[3], a[3], r[3];
            const double len = sqrt(z);
            for (int k = 0; k < 3; k++) {
                nn[k] = d[k] / len;
                a[k] = m->start[k] - m->axis_point[k];
            }
            const double dot = a[0] * nn[0] + a[1] * nn[1] + a[2] * nn[2];
            for (int k = 0; k < 3; k++) r[k] = a[k] - dot * nn[k];
            const double spin_radius = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
            if (!(spin_radius > 0)) return refuse(i, "the spin's radius is zero (start lies on the axis)");
            for (int k = 0; k < 3; k++) m->spin_axis[k] = nn[k], m->spin_offset[k] = a[k];
            m->spin_w = m->speed / spin_radius;
        }
        m->prepared = 1;
    }
    return LSCQP_OK;
}

extern "C" int lscqp_obstacles_advance_device(lscqp_handle h, const lscqp_obstacle_model* d_models, int32_t n_dyn, double time_step, int32_t* d_clock,
                                              lscqp_obstacle* d_obstacles, void* stream) {
    if (!h) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null handle");
    if (n_dyn < 0 || !(time_step > 0) || !(time_step < 1e6))
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "inconsistent sizes (n_dyn >= 0 and a positive, finite time_step required)");
    if (n_dyn > lscqp_max_obstacles(h))
        return lscqp_set_error_(LSCQP_ERR_UNSUPPORTED, "n_dyn exceeds the largest compiled kernel instance of the shape (lscqp_max_obstacles)");
    if (n_dyn == 0) return LSCQP_OK;
    if (!d_models || !d_clock || !d_obstacles) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null buffer");
    if (const int rc = lscqp_need_device_()) return rc;
    const int64_t step_ns = (int64_t)llround(time_step * 1e9);  // ros::Duration(time_step): whole nanoseconds
    hipLaunchKernelGGL(lscobstacle::obstacle_advance_kernel, dim3(1), dim3(lscobstacle::kThreads), 0, (hipStream_t)stream, d_models, (int)n_dyn, step_ns,
                       d_clock, d_obstacles);
    return lscqp_launch_result_(hipGetLastError());
}
