// lscobstacle.hip — how the mission's dynamic obstacles move, on the device, gfx950 only: the device analogue of
//   ObstacleGenerator::update(t, 0)      reference include/obstacle_generator.hpp:28-35, 95-110 (no observer noise)
//   StraightObstacle / PatrolObstacle / SpinObstacle::getObstacle   include/obstacle.hpp:83-264
// One kernel moves the whole obstacle table of a plan by one replan; lscplan.hip puts it in front of its chain.  The per-leg
// constants of StraightObstacle's constructor are made once on the host (lscqp_obstacle_model_prepare: no device needed), in the
// reference's own arithmetic: point3d is octomath::Vector3, three FLOATS -- Vector3::distance is the double square root of the double
// sum of squared float differences, normalized() divides by (float)norm(), norm() is the double square root of a float sum of squares,
// and `n * 0.5 * max_acc * t * t` is four Vector3::operator*(float) in a row.  Nothing here may contract a multiply and an add.
// A second kernel, in front of that one, moves the entries whose next state needs more than the time (obstacle_drive_kernel below):
//   ChasingObstacle / GaussianObstacle::getObstacle   include/obstacle.hpp:267-469
// This file has no object of its own: lscplan.hip includes it (as lscsfc_tp.hip includes lscsfc.hip), so that it is built with
// the chain that launches its kernel.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

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

// t of replan r: r steps of ros::Duration(time_step) -- step_ns whole nanoseconds each -- then Duration::toSec()
__host__ __device__ inline double clock_seconds(int32_t r, int64_t step_ns) {
#pragma clang fp contract(off)
    const int64_t ns = (int64_t)r * step_ns;
    return (double)(ns / 1000000000LL) + 1e-9 * (double)(ns % 1000000000LL);
}

// One slice of the table at time t: thread i takes entries i, i + 64, ...  HELD entries are not written.
__device__ __forceinline__ void advance_slice(const lscqp_obstacle_model* __restrict__ models, lscqp_obstacle* __restrict__ table, int n, double t) {
#pragma clang fp contract(off)
    for (int oi = threadIdx.x; oi < n; oi += kThreads) {
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
}

// One workgroup per table.  MIS: the table is mission-major (include/lscqp.h, "a mission's own obstacles"), workgroup k advances the slice
// [ooff[k], ooff[k + 1]) by the clock word clock[k] and reads or writes no word of another mission; a mission without obstacles still
// counts its clock.  Otherwise: the one table of n_dyn entries and the one clock word.  The clock word is read by every thread before the
// barrier and written by thread 0 behind it.
template <bool MIS>
__global__ __launch_bounds__(kThreads) void obstacle_advance_kernel(const lscqp_obstacle_model* __restrict__ models, const int32_t* __restrict__ ooff, int n_dyn,
                                                                     int64_t step_ns, int32_t* clock, lscqp_obstacle* __restrict__ table) {
#pragma clang fp contract(off)
    const int k = MIS ? blockIdx.x : 0;
    const int32_t r = clock[k];
    const int base = MIS ? ooff[k] : 0, n = MIS ? ooff[k + 1] - base : n_dyn;
    advance_slice(models + base, table + base, n, clock_seconds(r, step_ns));
    __syncthreads();
    if (threadIdx.x == 0) clock[k] = r + 1;
}

// ---- chasing and gaussian obstacles (include/lscqp.h, "chasing and gaussian obstacles"): ChasingObstacle::getChasingObstacle :313-363,
// GaussianObstacle::getGaussianObstacle :424-468.  The same functions run in obstacle_drive_kernel and in lscqp_obstacle_drive_host.

struct D3 {
    double x, y, z;
};

// |v| of an Eigen::Vector3d as this library defines it: sqrt((x x + y y) + z z)
__host__ __device__ inline double norm3(D3 v) {
#pragma clang fp contract(off)
    return sqrt((v.x * v.x + v.y * v.y) + v.z * v.z);
}

// an entry as the previous replan left it: what a chaser sees of the others (and of itself)
struct Staged {
    double px, py, pz, radius;
};

// getChasingObstacle with current_state = (own staged position, `vel`) and dt = t - t_last_called; goal: the goal point as point3d
__host__ __device__ inline void chasing_step(const lscqp_obstacle_model& m, const lscqp_obstacle_drive& d, F3 goal, const Staged* prev, int n_dyn, int self,
                                             double dt, F3* pos, F3* vel) {
#pragma clang fp contract(off)
    const F3 p{(float)prev[self].px, (float)prev[self].py, (float)prev[self].pz};
    D3 a{d.gamma_target * (double)(goal.x - p.x), d.gamma_target * (double)(goal.y - p.y), d.gamma_target * (double)(goal.z - p.z)};
    D3 v{(double)vel->x, (double)vel->y, (double)vel->z};
    for (int oj = 0; oj < n_dyn; oj++) {
        if (oj == self) continue;
        const D3 dl{(double)((float)prev[oj].px - p.x), (double)((float)prev[oj].py - p.y), (double)((float)prev[oj].pz - p.z)};
        const double dist = norm3(dl);
        if (dist < 1e-5) continue;  // SP_EPSILON_FLOAT
        const double q_star = 2 * (m.radius + prev[oj].radius);
        if (dist < q_star) {
            const double s = d.gamma_obs * (1 - dist / q_star) * (1 / (dist * q_star));
            a.x += s * (-(dl.x / dist)), a.y += s * (-(dl.y / dist)), a.z += s * (-(dl.z / dist));
        }
    }
    const double a_max = m.max_acc - 0.01, na = norm3(a);
    if (na > a_max) a = D3{a.x / na * a_max, a.y / na * a_max, a.z / na * a_max};
    v = D3{v.x + a.x * dt, v.y + a.y * dt, v.z + a.z * dt};
    const double nv = norm3(v);
    if (nv > d.max_vel) v = D3{v.x / nv * d.max_vel, v.y / nv * d.max_vel, v.z / nv * d.max_vel};
    *pos = F3{(float)((double)p.x + v.x * dt), (float)((double)p.y + v.y * dt), (float)((double)p.z + v.z * dt)};
    *vel = F3{(float)v.x, (float)v.y, (float)v.z};
}

// one pass of getGaussianObstacle's loop body over dt
__host__ __device__ inline void gaussian_cycle(lscqp_obstacle_drive_state* c, D3 acc, double dt, double max_vel) {
#pragma clang fp contract(off)
    const D3 v{c->v[0], c->v[1], c->v[2]};
    const D3 v_next{v.x + acc.x * dt, v.y + acc.y * dt, v.z + acc.z * dt};
    if (norm3(v_next) > max_vel) {  // "If v is over max_vel then ignore acc"
        c->position[0] = (float)((double)c->position[0] + v.x * dt);
        c->position[1] = (float)((double)c->position[1] + v.y * dt);
        c->position[2] = (float)((double)c->position[2] + v.z * dt);
    } else {
        c->position[0] = (float)((double)c->position[0] + (v.x * dt + 0.5 * acc.x * dt * dt));
        c->position[1] = (float)((double)c->position[1] + (v.y * dt + 0.5 * acc.y * dt * dt));
        c->position[2] = (float)((double)c->position[2] + (v.z * dt + 0.5 * acc.z * dt * dt));
        c->velocity[0] = (float)((double)c->velocity[0] + acc.x * dt);
        c->velocity[1] = (float)((double)c->velocity[1] + acc.y * dt);
        c->velocity[2] = (float)((double)c->velocity[2] + acc.z * dt);
        c->v[0] = v_next.x, c->v[1] = v_next.y, c->v[2] = v_next.z;
    }
}

// getGaussianObstacle(t) from the checkpoint: whole cycles i_done .. n - 1 on the checkpoint, the partial one on a copy.  Returns whether the
// history ended (an index at or past history_len, or outside the table, was asked for: zero acceleration)
__host__ __device__ inline bool gaussian_at(const lscqp_obstacle_model& m, const lscqp_obstacle_drive& d, const double* hist, int n_history,
                                            lscqp_obstacle_drive_state* ckpt, double t, F3* pos, F3* vel) {
#pragma clang fp contract(off)
    const double cycle = d.acc_update_cycle;
    const double q = floor((t + 1e-5) / cycle);
    const int n = q < 0 ? 0 : (q > 2147483646.0 ? 2147483646 : (int)q);  // (int n = floor(..) of the reference, kept inside an int)
    lscqp_obstacle_drive_state c = *ckpt;
    if (c.i_done <= 0 || c.i_done > n) {  // a zeroed checkpoint, or one ahead of a clock that was written backwards: from `start`
        c.i_done = 0, c.reserved = 0;
        for (int k = 0; k < 3; k++) {
            c.position[k] = (float)m.start[k];
            c.velocity[k] = (float)d.initial_vel[k];
            c.v[k] = (double)(float)d.initial_vel[k];
        }
    }
    bool ended = false;
    auto acc_of = [&](int i) {
        const int64_t at = (int64_t)d.history_first + i;
        if (i >= d.history_len || at < 0 || at >= n_history) {
            ended = true;
            return D3{0.0, 0.0, 0.0};
        }
        return D3{hist[at * 3 + 0], hist[at * 3 + 1], hist[at * 3 + 2]};
    };
    for (; c.i_done < n; c.i_done++) gaussian_cycle(&c, acc_of(c.i_done), cycle, d.max_vel);
    if (c.i_done != ckpt->i_done) *ckpt = c;
    gaussian_cycle(&c, acc_of(n), t - n * cycle, d.max_vel);
    *pos = F3{c.position[0], c.position[1], c.position[2]};
    *vel = F3{c.velocity[0], c.velocity[1], c.velocity[2]};
    return ended;
}

// One driven entry by one replan: `prev` holds EVERY entry as the previous replan left it, so no entry written here is read by another
__host__ __device__ inline void drive_entry(const lscqp_obstacle_model* models, const lscqp_obstacle_drive* drives, int n_dyn, const double* hist,
                                            int n_history, const double* state, int64_t n_total, lscqp_obstacle_drive_state* ckpt, double t, double t_last,
                                            const Staged* prev, int oi, lscqp_obstacle* table) {
#pragma clang fp contract(off)
    const lscqp_obstacle_drive& d = drives[oi];
    if (d.kind != LSCQP_DRIVE_CHASING && d.kind != LSCQP_DRIVE_GAUSSIAN) return;
    const lscqp_obstacle_model& m = models[oi];
    lscqp_obstacle* o = table + oi;
    F3 p, v;
    int32_t flags = 0;
    if (d.kind == LSCQP_DRIVE_CHASING) {
        const int64_t ta = d.target_agent;
        const double* g = (state != nullptr && ta >= 0 && ta < n_total) ? state + ta * 9 : d.goal;
        v = F3{(float)o->velocity[0], (float)o->velocity[1], (float)o->velocity[2]};
        chasing_step(m, d, F3{(float)g[0], (float)g[1], (float)g[2]}, prev, n_dyn, oi, t - t_last, &p, &v);
    } else if (gaussian_at(m, d, hist, hist != nullptr ? n_history : 0, ckpt + oi, t, &p, &v)) {
        flags = LSCQP_OBSTACLE_HISTORY_ENDED;
    }
    o->position[0] = (double)p.x, o->position[1] = (double)p.y, o->position[2] = (double)p.z;
    o->velocity[0] = (double)v.x, o->velocity[1] = (double)v.y, o->velocity[2] = (double)v.z;
    o->radius = m.radius, o->downwash = m.downwash, o->max_acc = m.max_acc;
    o->type = 0;  // DYNAMICOBSTACLE (ObstacleBase::getObstacle)
    o->reserved = flags;
}

// One workgroup per table, as obstacle_advance_kernel takes them; thread i takes entries i, i + 64, ... of its table.  Every entry's previous
// position and radius go to LDS first (dynamic LDS: the largest table's count of Staged records); behind the barrier the table is only
// written, and an entry's own velocity is read by the one thread that writes it.  drive_entry gets the table's base pointers, count and local
// index: a chaser sees the obstacles of its own table and no other.  target_agent stays a global id into `state`; the history table is one
// for all.  The clock word is read, never written: the advance behind this kernel counts it.
template <bool MIS>
__global__ __launch_bounds__(kThreads) void obstacle_drive_kernel(const lscqp_obstacle_model* __restrict__ models, const lscqp_obstacle_drive* __restrict__ drives,
                                                                   const int32_t* __restrict__ ooff, int n_dyn, const double* __restrict__ hist, int n_history,
                                                                   const double* __restrict__ state, int64_t n_total, lscqp_obstacle_drive_state* __restrict__ ckpt,
                                                                   int64_t step_ns, const int32_t* __restrict__ clock, lscqp_obstacle* table) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char drive_lds[];
    Staged* prev = (Staged*)drive_lds;
    const int k = MIS ? blockIdx.x : 0;
    const int base = MIS ? ooff[k] : 0, n = MIS ? ooff[k + 1] - base : n_dyn;
    const int32_t r = clock[k];
    const double t = clock_seconds(r, step_ns), t_last = r > 0 ? clock_seconds(r - 1, step_ns) : 0.0;
    lscqp_obstacle* mine = table + base;
    for (int oi = threadIdx.x; oi < n; oi += kThreads) prev[oi] = Staged{mine[oi].position[0], mine[oi].position[1], mine[oi].position[2], mine[oi].radius};
    __syncthreads();
    for (int oi = threadIdx.x; oi < n; oi += kThreads)
        drive_entry(models + base, drives + base, n, hist, n_history, state, n_total, ckpt + base, t, t_last, prev, oi, mine);
}

constexpr size_t kDriveLdsMax = 64 * 1024;  // (2048 entries: far beyond lscqp_max_obstacles of any class)

// the offset list of a table per mission, as the host gives it: K + 1 values, non-decreasing from 0 to n_dyn_total, no mission with more
// than lscqp_max_obstacles(h) entries.  *largest: the largest mission's count
inline int check_obstacle_offsets(lscqp_handle h, int32_t n_missions, const int32_t* ooff, int32_t n_dyn_total, int32_t* largest) {
    *largest = 0;
    if (n_missions < 1 || !ooff) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "a table per mission needs n_missions >= 1 and its obstacle_offsets");
    if (ooff[0] != 0) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "obstacle_offsets[0] must be 0");
    for (int32_t k = 0; k < n_missions; k++) {
        if (ooff[k + 1] < ooff[k]) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "obstacle_offsets must not decrease");
        if (ooff[k + 1] - ooff[k] > *largest) *largest = ooff[k + 1] - ooff[k];
    }
    if (ooff[n_missions] != n_dyn_total) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "obstacle_offsets[n_missions] must be n_dyn_total");
    if (*largest > lscqp_max_obstacles(h) || (size_t)*largest * sizeof(Staged) > kDriveLdsMax)
        return lscqp_set_error_(LSCQP_ERR_UNSUPPORTED, "a mission's obstacle count exceeds the largest compiled kernel instance of the shape (lscqp_max_obstacles)");
    return LSCQP_OK;
}

// behind an entry's checks: the device, the step in whole nanoseconds (ros::Duration(time_step)), one workgroup per table
template <bool MIS>
int launch_advance(const lscqp_obstacle_model* models, int n_tables, const int32_t* ooff, int n_dyn, double time_step, int32_t* clock, lscqp_obstacle* table,
                   void* stream) {
    if (const int rc = lscqp_need_device_()) return rc;
    const int64_t step_ns = (int64_t)llround(time_step * 1e9);
    hipLaunchKernelGGL(obstacle_advance_kernel<MIS>, dim3((unsigned)n_tables), dim3(kThreads), 0, (hipStream_t)stream, models, ooff, n_dyn, step_ns, clock, table);
    return lscqp_launch_result_(hipGetLastError());
}

// (largest: the largest table's count, the Staged records of LDS)
template <bool MIS>
int launch_drive(const lscqp_obstacle_model* models, const lscqp_obstacle_drive* drives, int n_tables, const int32_t* ooff, int n_dyn, int largest,
                 const double* hist, int n_history, const double* state, int64_t n_total, lscqp_obstacle_drive_state* ckpt, double time_step, const int32_t* clock,
                 lscqp_obstacle* table, void* stream) {
    if (const int rc = lscqp_need_device_()) return rc;
    const int64_t step_ns = (int64_t)llround(time_step * 1e9);
    hipLaunchKernelGGL(obstacle_drive_kernel<MIS>, dim3((unsigned)n_tables), dim3(kThreads), (size_t)largest * sizeof(Staged), (hipStream_t)stream, models, drives, ooff,
                       n_dyn, hist, n_history, state, n_total, ckpt, step_ns, clock, table);
    return lscqp_launch_result_(hipGetLastError());
}

// the buffers every drive entry needs once there is an entry to move
inline bool drive_buffer_missing(const void* models, const void* drives, const double* hist, int32_t n_history, const double* state, int64_t n_total, const void* ckpt,
                                 const void* clock, const void* table) {
    return !models || !drives || !ckpt || !clock || !table || (n_history > 0 && !hist) || (n_total > 0 && !state);
}

inline int refuse_drive(int i, const char* what) {
    char msg[240];
    snprintf(msg, sizeof msg, "lscqp_obstacle_drive_check: model %d: %s", i, what);
    return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, msg);
}

// the argument checks the device and the host entry share (the advance entry's, and the tables the drives index)
inline int drive_args(lscqp_handle h, const void* models, const void* drives, int32_t n_dyn, const double* hist, int32_t n_history, const double* state,
                      int64_t n_total, const void* ckpt, double time_step, const void* clock, const void* table, bool* empty) {
    *empty = false;
    if (!h) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null handle");
    if (n_dyn < 0 || n_history < 0 || n_total < 0 || !(time_step > 0) || !(time_step < 1e6))
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT,
                                "inconsistent sizes (n_dyn >= 0, n_history >= 0, n_total >= 0 and a positive, finite time_step required)");
    if (n_dyn > lscqp_max_obstacles(h) || (size_t)n_dyn * sizeof(Staged) > kDriveLdsMax)
        return lscqp_set_error_(LSCQP_ERR_UNSUPPORTED, "n_dyn exceeds the largest compiled kernel instance of the shape (lscqp_max_obstacles)");
    if (n_dyn == 0) {
        *empty = true;
        return LSCQP_OK;
    }
    if (drive_buffer_missing(models, drives, hist, n_history, state, n_total, ckpt, clock, table)) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null buffer");
    return LSCQP_OK;
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
    return lscobstacle::launch_advance<false>(d_models, 1, nullptr, n_dyn, time_step, d_clock, d_obstacles, stream);
}

extern "C" int lscqp_obstacle_drive_check(const lscqp_obstacle_model* models, const lscqp_obstacle_drive* drives, int32_t n, int32_t n_history,
                                          int64_t n_total) {
    using namespace lscobstacle;
    if (n < 0 || n_history < 0 || n_total < 0) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "negative size");
    if (n == 0) return LSCQP_OK;
    if (!models || !drives) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null buffer");
    for (int i = 0; i < n; i++) {
        const lscqp_obstacle_drive& d = drives[i];
        const lscqp_obstacle_model& m = models[i];
        if (d.kind == LSCQP_DRIVE_NONE) continue;
        if (d.kind != LSCQP_DRIVE_CHASING && d.kind != LSCQP_DRIVE_GAUSSIAN)
            return refuse_drive(i, "kind must be LSCQP_DRIVE_NONE, _CHASING or _GAUSSIAN");
        if (m.kind != LSCQP_OBSTACLE_HELD) return refuse_drive(i, "a drive needs an LSCQP_OBSTACLE_HELD model (the advance moves every other kind)");
        if (!isfinite(d.max_vel) || !isfinite(d.gamma_target) || !isfinite(d.gamma_obs) || !finite3(d.goal) || !finite3(d.initial_vel) ||
            !isfinite(d.acc_update_cycle) || !isfinite(m.radius) || !isfinite(m.max_acc) || !isfinite(m.downwash) || !finite3(m.start))
            return refuse_drive(i, "a field is not finite (max_vel, gamma_target, gamma_obs, goal, initial_vel, acc_update_cycle; the model's radius, max_acc, downwash, start)");
        if (!(d.max_vel > 0)) return refuse_drive(i, "max_vel <= 0");
        if (d.kind == LSCQP_DRIVE_CHASING) {
            if (d.target_agent < -1 || d.target_agent >= n_total) return refuse_drive(i, "target_agent outside [-1, n_total)");
            if (!(m.max_acc > 0.01)) return refuse_drive(i, "max_acc <= 0.01 (a chaser's acceleration is clamped to max_acc - 0.01)");
        } else {
            if (!(d.acc_update_cycle > 0)) return refuse_drive(i, "acc_update_cycle <= 0");
            if (d.history_len <= 0) return refuse_drive(i, "the history slice is empty (history_len >= 1 required)");
            if (d.history_first < 0 || (int64_t)d.history_first + d.history_len > n_history)
                return refuse_drive(i, "the history slice lies outside [0, n_history)");
        }
    }
    return LSCQP_OK;
}

extern "C" int lscqp_obstacles_drive_device(lscqp_handle h, const lscqp_obstacle_model* d_models, const lscqp_obstacle_drive* d_drives, int32_t n_dyn,
                                            const double* d_acc_history, int32_t n_history, const double* d_state, int64_t n_total,
                                            lscqp_obstacle_drive_state* d_drive_state, double time_step, const int32_t* d_clock,
                                            lscqp_obstacle* d_obstacles, void* stream) {
    bool empty = false;
    if (const int rc = lscobstacle::drive_args(h, d_models, d_drives, n_dyn, d_acc_history, n_history, d_state, n_total, d_drive_state, time_step, d_clock,
                                               d_obstacles, &empty))
        return rc;
    if (empty) return LSCQP_OK;
    return lscobstacle::launch_drive<false>(d_models, d_drives, 1, nullptr, n_dyn, n_dyn, d_acc_history, n_history, d_state, n_total, d_drive_state, time_step, d_clock,
                                            d_obstacles, stream);
}

extern "C" int lscqp_obstacle_drive_host(lscqp_handle h, const lscqp_obstacle_model* models, const lscqp_obstacle_drive* drives, int32_t n_dyn,
                                         const double* acc_history, int32_t n_history, const double* state, int64_t n_total,
                                         lscqp_obstacle_drive_state* drive_state, double time_step, const int32_t* clock, lscqp_obstacle* obstacles,
                                         void* stream) {
    using namespace lscobstacle;
    (void)stream;
    bool empty = false;
    if (const int rc = drive_args(h, models, drives, n_dyn, acc_history, n_history, state, n_total, drive_state, time_step, clock, obstacles, &empty)) return rc;
    if (empty) return LSCQP_OK;
    const int64_t step_ns = (int64_t)llround(time_step * 1e9);
    const int32_t r = *clock;
    const double t = clock_seconds(r, step_ns), t_last = r > 0 ? clock_seconds(r - 1, step_ns) : 0.0;
    std::vector<Staged> prev((size_t)n_dyn);
    for (int oi = 0; oi < n_dyn; oi++) prev[(size_t)oi] = Staged{obstacles[oi].position[0], obstacles[oi].position[1], obstacles[oi].position[2], obstacles[oi].radius};
    for (int oi = 0; oi < n_dyn; oi++) drive_entry(models, drives, n_dyn, acc_history, n_history, state, n_total, drive_state, t, t_last, prev.data(), oi, obstacles);
    return LSCQP_OK;
}

extern "C" int lscqp_obstacles_advance_missions_device(lscqp_handle h, const lscqp_obstacle_model* d_models, int32_t n_missions,
                                                       const int32_t* obstacle_offsets, const int32_t* d_obstacle_offsets, int32_t n_dyn_total,
                                                       double time_step, int32_t* d_clock, lscqp_obstacle* d_obstacles, void* stream) {
    if (!h) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null handle");
    if (n_missions < 0 || n_dyn_total < 0 || !(time_step > 0) || !(time_step < 1e6))
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "inconsistent sizes (n_missions >= 0, n_dyn_total >= 0 and a positive, finite time_step required)");
    if (n_missions == 0) return LSCQP_OK;
    int32_t largest = 0;
    if (const int rc = lscobstacle::check_obstacle_offsets(h, n_missions, obstacle_offsets, n_dyn_total, &largest)) return rc;
    // (a partition none of whose missions has an obstacle still counts its clocks: no table is asked for)
    if (!d_obstacle_offsets || !d_clock || (n_dyn_total > 0 && (!d_models || !d_obstacles))) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null buffer");
    return lscobstacle::launch_advance<true>(d_models, n_missions, d_obstacle_offsets, n_dyn_total, time_step, d_clock, d_obstacles, stream);
}

extern "C" int lscqp_obstacles_drive_missions_device(lscqp_handle h, const lscqp_obstacle_model* d_models, const lscqp_obstacle_drive* d_drives,
                                                     int32_t n_missions, const int32_t* obstacle_offsets, const int32_t* d_obstacle_offsets,
                                                     int32_t n_dyn_total, const double* d_acc_history, int32_t n_history, const double* d_state,
                                                     int64_t n_total, lscqp_obstacle_drive_state* d_drive_state, double time_step,
                                                     const int32_t* d_clock, lscqp_obstacle* d_obstacles, void* stream) {
    if (!h) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null handle");
    if (n_missions < 0 || n_dyn_total < 0 || n_history < 0 || n_total < 0 || !(time_step > 0) || !(time_step < 1e6))
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT,
                                "inconsistent sizes (n_missions >= 0, n_dyn_total >= 0, n_history >= 0, n_total >= 0 and a positive, finite time_step required)");
    if (n_missions == 0) return LSCQP_OK;
    int32_t largest = 0;
    if (const int rc = lscobstacle::check_obstacle_offsets(h, n_missions, obstacle_offsets, n_dyn_total, &largest)) return rc;
    if (n_dyn_total == 0) return LSCQP_OK;  // (nothing to move, and the clocks are the advance's to count)
    if (!d_obstacle_offsets || lscobstacle::drive_buffer_missing(d_models, d_drives, d_acc_history, n_history, d_state, n_total, d_drive_state, d_clock, d_obstacles))
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null buffer");
    return lscobstacle::launch_drive<true>(d_models, d_drives, n_missions, d_obstacle_offsets, n_dyn_total, largest, d_acc_history, n_history, d_state, n_total,
                                           d_drive_state, time_step, d_clock, d_obstacles, stream);
}
