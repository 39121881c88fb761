// lscpatrol.hip — patrol missions (include/lscqp.h, "patrol missions"), gfx950 only: the device analogue of
//   AgentManager::planningStateTransition, PATROL branch   reference src/agent_manager.cpp:225-240
//   MultiSyncSimulator's PlannerState::PATROL               src/multi_sync_simulator.cpp:57-61, and isFinished :401-404 (never)
// Two kernels, both enqueued by lscplan.hip directly behind the waypoint decision: `patrol_kernel` swaps the desired goal and the start point
// of every agent that has arrived, `field_exchange_kernel` hands such an agent the distance field of its new leg.  The distance is the
// mission record's (lscqp_point3d.hpp: norm_of_difference), compared the other way round: the record finishes a GOTO mission unless
// distance > threshold, a patrolling agent turns if distance < threshold -- at equality the one is finished and the other does not turn.
// This file has no object of its own: lscplan.hip includes it (as it includes lscobstacle.hip), so that it is built with the chain that
// launches its kernels.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "../../include/lscqp.h"
#include "lscqp_internal.hpp"
#include "lscqp_point3d.hpp"

namespace lscpatrol {

constexpr int kThreads = 64;

// one agent's transition; the same function runs in patrol_kernel and in lscqp_patrol_host
__host__ __device__ inline void transition(const double* state, double* desired, double* start, double goal_threshold, int dim, double z_2d,
                                           int32_t* legs, int32_t* swapped, int64_t a) {
    // agent.current_state.position is a point3d, and a 2-D mission flies in its plane whatever the buffer's third word holds
    const float p[3] = {(float)state[a * 9 + 0], (float)state[a * 9 + 1], dim == 3 ? (float)state[a * 9 + 2] : (float)z_2d};
    double* g = desired + a * 3;
    double* s = start + a * 3;
    const float gf[3] = {(float)g[0], (float)g[1], (float)g[2]};
    const bool turn = lscqp::norm_of_difference(gf, p) < goal_threshold;  // desired_goal_point.distance(position) < param.goal_threshold
    if (turn) {
        for (int k = 0; k < 3; k++) {
            const double t = g[k];
            g[k] = s[k];
            s[k] = t;
        }
        legs[a] += 1;
    }
    swapped[a] = turn ? 1 : 0;  // (written either way: a replayed graph carries no stale flag)
}

// One thread per agent; no LDS, no atomics: a thread reads and writes its own agent's words alone.
__global__ __launch_bounds__(kThreads) void patrol_kernel(int64_t n, const double* __restrict__ state, double* __restrict__ desired,
                                                          double* __restrict__ start, double goal_threshold, int dim, double z_2d,
                                                          int32_t* __restrict__ legs, int32_t* __restrict__ swapped) {
    const int64_t a = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (a >= n) return;
    transition(state, desired, start, goal_threshold, dim, z_2d, legs, swapped, a);
}

// The fields of an agent that turned.  Grid (agent, chunk): workgroup (a, c) owns words [c * kChunk, (c + 1) * kChunk) of agent a's slice in
// both buffers, a thread kUnroll of them, kExThreads apart; it reads both words and writes both, and nobody else touches them.  A workgroup
// whose agent did not turn returns after one load of the same word by every lane.  Every access is ONE dword: a slice starts at
// a * nodes * 4 bytes, which is only 4-byte aligned when `nodes` is odd, so there is no wider access whose head and tail would need care.
constexpr int kExThreads = 256, kUnroll = 4, kChunk = kExThreads * kUnroll;
constexpr int64_t kMaxChunks = 65535;  // gridDim.y

__global__ __launch_bounds__(kExThreads) void field_exchange_kernel(int64_t nodes, const int32_t* __restrict__ swapped, int32_t* __restrict__ field,
                                                                     int32_t* __restrict__ other, int32_t* __restrict__ init_d,
                                                                     int32_t* __restrict__ init_d_other) {
    const int64_t a = blockIdx.x;
    if (swapped[a] == 0) return;
    const size_t base = (size_t)a * (size_t)nodes;
    const int64_t first = (int64_t)blockIdx.y * kChunk + threadIdx.x;
    int32_t u[kUnroll] = {}, v[kUnroll] = {};
#pragma unroll
    for (int k = 0; k < kUnroll; k++) {
        const int64_t i = first + (int64_t)k * kExThreads;
        if (i < nodes) u[k] = field[base + (size_t)i], v[k] = other[base + (size_t)i];
    }
#pragma unroll
    for (int k = 0; k < kUnroll; k++) {
        const int64_t i = first + (int64_t)k * kExThreads;
        if (i < nodes) field[base + (size_t)i] = v[k], other[base + (size_t)i] = u[k];
    }
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        const int32_t d = init_d[a];
        init_d[a] = init_d_other[a];
        init_d_other[a] = d;
    }
}

// what PATROL compares against: param.goal_threshold, finite and not negative (0 never turns anyone: no distance is < 0)
inline int check_threshold(const char* who, double goal_threshold) {
    if (!isfinite(goal_threshold) || goal_threshold < 0)
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, (std::string(who) + ": goal_threshold must be finite and >= 0").c_str());
    return LSCQP_OK;
}

// the argument checks the device and the host entry share
inline int patrol_args(const char* who, lscqp_handle h, int64_t n, const void* state, const void* desired, const void* start, double goal_threshold,
                       int32_t dim, double z_2d, const void* legs, const void* swapped) {
    if (!h) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null handle");
    if (n < 0 || n > 0x7fffffff) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, (std::string(who) + ": 0 <= n < 2^31 required").c_str());
    if (dim != 2 && dim != 3) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, (std::string(who) + ": dim must be 2 or 3").c_str());
    if (const int rc = check_threshold(who, goal_threshold)) return rc;
    if (!isfinite(z_2d)) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, (std::string(who) + ": z_2d is not finite").c_str());
    if (n > 0 && (!state || !desired || !start || !legs || !swapped)) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null buffer");
    if (n > 0 && desired == start)
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, (std::string(who) + ": the desired goals and the start points are one buffer").c_str());
    return LSCQP_OK;
}

}  // namespace lscpatrol

extern "C" int lscqp_patrol_check(const lscqp_patrol_desc* desc, int64_t n_agents, int64_t n_total) {
    if (!desc) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_patrol_check: null descriptor");
    if (const int rc = lscpatrol::check_threshold("lscqp_patrol_check", desc->goal_threshold)) return rc;
    if (n_agents < 0 || n_total <= 0) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_patrol_check: n_agents >= 0 and n_total > 0 required");
    if (n_agents != n_total)
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT,
                                "lscqp_patrol_check: a patrol needs every agent on this device (n_agents == n_total): the transition writes every agent's goal");
    return LSCQP_OK;
}

extern "C" int lscqp_patrol_device(lscqp_handle h, int64_t n, const double* d_state, double* d_desired, double* d_start, double goal_threshold,
                                   int32_t dim, double z_2d, int32_t* d_legs, int32_t* d_swapped, void* stream) {
    if (const int rc = lscpatrol::patrol_args("lscqp_patrol_device", h, n, d_state, d_desired, d_start, goal_threshold, dim, z_2d, d_legs, d_swapped)) return rc;
    if (n == 0) return LSCQP_OK;
    if (const int rc = lscqp_need_device_()) return rc;
    const unsigned nb = (unsigned)((n + lscpatrol::kThreads - 1) / lscpatrol::kThreads);
    hipLaunchKernelGGL(lscpatrol::patrol_kernel, dim3(nb), dim3(lscpatrol::kThreads), 0, (hipStream_t)stream, n, d_state, d_desired, d_start, goal_threshold,
                       (int)dim, z_2d, d_legs, d_swapped);
    return lscqp_launch_result_(hipGetLastError());
}

extern "C" int lscqp_patrol_host(lscqp_handle h, int64_t n, const double* state, double* desired, double* start, double goal_threshold, int32_t dim,
                                 double z_2d, int32_t* legs, int32_t* swapped, void* stream) {
    (void)stream;
    if (const int rc = lscpatrol::patrol_args("lscqp_patrol_host", h, n, state, desired, start, goal_threshold, dim, z_2d, legs, swapped)) return rc;
    for (int64_t a = 0; a < n; a++) lscpatrol::transition(state, desired, start, goal_threshold, (int)dim, z_2d, legs, swapped, a);
    return LSCQP_OK;
}

extern "C" int lscqp_field_exchange_device(int64_t n, int64_t nodes, const int32_t* d_swapped, int32_t* d_field, int32_t* d_field_other,
                                           int32_t* d_init_d, int32_t* d_init_d_other, void* stream) {
    using namespace lscpatrol;
    if (n < 0 || n > 0x7fffffff || nodes <= 0)
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_field_exchange_device: 0 <= n < 2^31 and nodes > 0 required");
    const int64_t chunks = (nodes + kChunk - 1) / kChunk;
    if (chunks > kMaxChunks)
        return lscqp_set_error_(LSCQP_ERR_UNSUPPORTED, "lscqp_field_exchange_device: a field of more than 65535 x 1024 nodes is not exchanged");
    if (n == 0) return LSCQP_OK;
    if (!d_swapped || !d_field || !d_field_other || !d_init_d || !d_init_d_other) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null buffer");
    if (d_field == d_field_other || d_init_d == d_init_d_other)
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_field_exchange_device: the two fields (or their init_d words) are one buffer");
    if (const int rc = lscqp_need_device_()) return rc;
    hipLaunchKernelGGL(field_exchange_kernel, dim3((unsigned)n, (unsigned)chunks), dim3(kExThreads), 0, (hipStream_t)stream, nodes, d_swapped, d_field,
                       d_field_other, d_init_d, d_init_d_other);
    return lscqp_launch_result_(hipGetLastError());
}
