// lscrecord.hip — the mission record (include/lscqp.h, "the mission record"), gfx950 only: the running figures of the reference's summary
// line per mission, accumulated on the device at the end of each replan, and the test that tells when a mission is over.
//   MultiSyncSimulator::isFinished          reference src/multi_sync_simulator.cpp:401-424
//   MultiSyncSimulator::getTotalDistance    :711-720 (the polyline through the logged sample points)
//   MultiSyncSimulator::update              :486-577 (minimum safety ratio, maximum excess ratios; per agent in lscpost.hip)
//   saveSummarizedResultAsCSV               :658-709 (what becomes of the figures)
// One workgroup per mission, its threads stride over the mission's agents: sample points, distance, and the partial figures of its agents,
// then ONE reduction across the workgroup (DPP moves within a wavefront, LDS across the four wavefronts, combined in wavefront order).  Every
// reduced figure is a sum of integers, a maximum, or a minimum whose ties go to the lowest agent id: the result does not depend on how the
// agents fall onto lanes.  A record may carry a flight log (include/lscqp.h, "the flight log"): a second kernel, below the record's, and an
// obstacle record (include/lscqp.h, "the obstacle record"): a third, below the log's.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/lscqp.h"
#include "lscpost_traj.hpp"
#include "lscqp_device.hpp"
#include "lscqp_internal.hpp"
#include "lscqp_point3d.hpp"


namespace lscrecord {

constexpr int kThreads = 256, kWaves = kThreads / 64;

struct Args {
    int M, dim, n_samples;
    double dt, record_time_step, time_step, z_2d, goal_threshold;
    int64_t n_total;
    const int64_t* off;  // [K + 1] or NULL: one mission [0, n_total)
    const lscqp_header* hdr;
    const double* x_all;
    const int32_t *status, *goal_status, *sfc_status, *valid, *in_range, *waypoint_updated;  // (waypoint_updated may be NULL)
    const lscqp_safety* safety;
    const float* goal;  // [n_total][3] desired goals, float32
    float* points;      // [n_total][n_samples][3]
    float* last;        // [n_total][3] the agent's last sample point of the previous replan
    double* dist;       // [n_total]
    lscqp_mission_record* rec;
    int32_t* unfinished;
};

// what a lane, a wavefront and the workgroup hold of the mission's agents in one replan.  Scalar fields only, listed once: small arrays
// indexed by loops stay in memory until the loops are unrolled, and by then the selects of `combine` have become selects of addresses
// (scratch instead of registers).
#define LSCREC_MAXIMA(X) X(vel_x) X(vel_y) X(vel_z) X(acc_x) X(acc_y) X(acc_z) /* excess ratios, never below 0 */
#define LSCREC_COUNTS(X) X(qp_failed) X(invalid) X(goal_failed) X(sfc_kept) X(waypoint) X(truncated) X(far) /* far: agents beyond the threshold */
struct Part {
    double ratio;      // least safety ratio, +inf: none
    int agent, other;  // ... the agent attaining it (lowest id on ties) and its closest agent; -1
#define X(f) double f;
    LSCREC_MAXIMA(X)
#undef X
#define X(f) int f;
    LSCREC_COUNTS(X)
#undef X
    int max_in_range;
};

__device__ __forceinline__ Part empty_part() {
    Part p;
    p.ratio = INFINITY, p.agent = -1, p.other = -1;
#define X(f) p.f = 0.0;
    LSCREC_MAXIMA(X)
#undef X
#define X(f) p.f = 0;
    LSCREC_COUNTS(X)
#undef X
    p.max_in_range = 0;
    return p;
}

// (ids compare as unsigned: -1, "none", loses every tie)
__device__ __forceinline__ void combine(Part& a, const Part& b) {
    // (`if`, not `take ? b.f : a.f`: a conditional between two lvalues is a choice of ADDRESS, which keeps both structs in memory)
    if (b.ratio < a.ratio || (b.ratio == a.ratio && (unsigned)b.agent < (unsigned)a.agent)) {
        a.ratio = b.ratio;
        a.agent = b.agent;
        a.other = b.other;
    }
#define X(f) \
    if (b.f > a.f) a.f = b.f;
    LSCREC_MAXIMA(X)
#undef X
#define X(f) a.f += b.f;
    LSCREC_COUNTS(X)
#undef X
    if (b.max_in_range > a.max_in_range) a.max_in_range = b.max_in_range;
}

// one DPP move of every field (lscqp_kernel.hpp: row_shr steps scan a row of 16 lanes, row_bcast:15 / :31 carry the rows' results across;
// lanes without a source receive the identity) and the combination with it
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_i32(int idn, int v) {
    return __builtin_amdgcn_update_dpp(idn, v, CTRL, ROW_MASK, 0xf, false);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_f64(double idn, double v) {
    const int lo = dpp_i32<CTRL, ROW_MASK>(__double2loint(idn), __double2loint(v));
    const int hi = dpp_i32<CTRL, ROW_MASK>(__double2hiint(idn), __double2hiint(v));
    return __hiloint2double(hi, lo);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ void dpp_step(Part& p) {
    Part q;
    q.ratio = dpp_f64<CTRL, ROW_MASK>(INFINITY, p.ratio);
    q.agent = dpp_i32<CTRL, ROW_MASK>(-1, p.agent);
    q.other = dpp_i32<CTRL, ROW_MASK>(-1, p.other);
#define X(f) q.f = dpp_f64<CTRL, ROW_MASK>(0.0, p.f);
    LSCREC_MAXIMA(X)
#undef X
#define X(f) q.f = dpp_i32<CTRL, ROW_MASK>(0, p.f);
    LSCREC_COUNTS(X)
#undef X
    q.max_in_range = dpp_i32<CTRL, ROW_MASK>(0, p.max_in_range);
    combine(p, q);
}
// lane 63 ends up with the wavefront's figures
__device__ __forceinline__ void wave_reduce(Part& p) {
    dpp_step<0x111, 0xf>(p);  // row_shr:1
    dpp_step<0x112, 0xf>(p);  // row_shr:2
    dpp_step<0x114, 0xf>(p);  // row_shr:4
    dpp_step<0x118, 0xf>(p);  // row_shr:8
    dpp_step<0x142, 0xa>(p);  // row_bcast:15 into rows 1 and 3
    dpp_step<0x143, 0xc>(p);  // row_bcast:31 into rows 2 and 3
}

// (a - b).norm() of octomath::Vector3 (lscqp_point3d.hpp: the patrol transition of lscpatrol.hip measures with the same function)
using lscqp::norm_of_difference;

__global__ __launch_bounds__(kThreads) void record_kernel(Args A) {
    __shared__ Part s_part[kWaves];
    const int k = blockIdx.x;
    lscqp_mission_record* R = A.rec + k;
    if (R->finished != 0) return;  // frozen (the whole workgroup: one word, the same for every lane)
    const int r = R->replans;      // this replan's index
    const int64_t lo = A.off ? A.off[k] : 0, hi = A.off ? A.off[k + 1] : A.n_total;
    const int nv = A.dim * 6 * A.M;
    Part p = empty_part();
    for (int64_t a = lo + threadIdx.x; a < hi; a += kThreads) {
        // sample points of the new plan, the polyline through them and the previous replan's last point
        float prev[3] = {0, 0, 0};
        if (r > 0) prev[0] = A.last[a * 3 + 0], prev[1] = A.last[a * 3 + 1], prev[2] = A.last[a * 3 + 2];
        double d = A.dist[a];
        float* pts = A.points + a * A.n_samples * 3;
        for (int s = 0; s < A.n_samples; s++) {
            float q[3];
            lscpost::position_at(A.M, A.dim, A.dt, s * A.record_time_step, A.z_2d, A.x_all + a * nv, q);
            pts[s * 3 + 0] = q[0], pts[s * 3 + 1] = q[1], pts[s * 3 + 2] = q[2];
            if (r > 0 || s > 0) d += norm_of_difference(q, prev);
            prev[0] = q[0], prev[1] = q[1], prev[2] = q[2];
        }
        A.dist[a] = d;
        A.last[a * 3 + 0] = prev[0], A.last[a * 3 + 1] = prev[1], A.last[a * 3 + 2] = prev[2];
        // the replan's figures of this agent (ascending ids within a lane: strict < keeps the lowest)
        Part q = empty_part();
        const lscqp_safety* S = A.safety + a;
        const lscqp_header* H = A.hdr + a;
        auto positive = [](double v) { return v > 0.0 ? v : 0.0; };
        q.ratio = S->safety_ratio, q.agent = (int)a, q.other = S->closest_agent;
        q.vel_x = positive(S->vel_excess_ratio[0]), q.vel_y = positive(S->vel_excess_ratio[1]), q.vel_z = positive(S->vel_excess_ratio[2]);
        q.acc_x = positive(S->acc_excess_ratio[0]), q.acc_y = positive(S->acc_excess_ratio[1]), q.acc_z = positive(S->acc_excess_ratio[2]);
        const int in_range = A.in_range[a];
        q.qp_failed = A.status[a] != LSCQP_STATUS_OPTIMAL;
        q.invalid = A.valid[a] == 0;
        q.goal_failed = A.goal_status[a] != 0;
        q.sfc_kept = A.sfc_status[a] == 0;
        q.waypoint = A.waypoint_updated ? A.waypoint_updated[a] != 0 : 0;
        q.truncated = in_range > H->n_obs;
        q.max_in_range = in_range > 0 ? in_range : 0;
        // isFinished: current_position.distance(desired_goal_point) > goal_threshold, on the state this replan started from
        const float p0[3] = {(float)H->p0[0], (float)H->p0[1], (float)H->p0[2]};
        const float g[3] = {A.goal[a * 3 + 0], A.goal[a * 3 + 1], A.goal[a * 3 + 2]};
        q.far = norm_of_difference(p0, g) > A.goal_threshold;
        combine(p, q);
    }
    wave_reduce(p);
    if ((threadIdx.x & 63) == 63) s_part[threadIdx.x >> 6] = p;
    __syncthreads();
    if (threadIdx.x != 0) return;
    p = s_part[0];
    for (int w = 1; w < kWaves; w++) combine(p, s_part[w]);
    if (p.ratio < R->safety_ratio_agent) {  // strict <: an earlier replan keeps a tie
        R->safety_ratio_agent = p.ratio;
        R->safety_replan = r, R->safety_agent = p.agent, R->safety_other = p.other;
    }
    const double ex[6] = {p.vel_x, p.vel_y, p.vel_z, p.acc_x, p.acc_y, p.acc_z};
    for (int i = 0; i < 3; i++) {
        if (ex[i] > R->vel_excess_ratio[i]) R->vel_excess_ratio[i] = ex[i];
        if (ex[3 + i] > R->acc_excess_ratio[i]) R->acc_excess_ratio[i] = ex[3 + i];
    }
    R->qp_failed += p.qp_failed;
    if (p.qp_failed > 0 && R->first_qp_failed_replan < 0) R->first_qp_failed_replan = r;
    R->invalid += p.invalid;
    R->goal_failed += p.goal_failed;
    R->sfc_kept += p.sfc_kept;
    R->waypoint_updates += p.waypoint;
    R->truncated += p.truncated;
    if (p.max_in_range > R->max_in_range) R->max_in_range = p.max_in_range;
    R->replans = r + 1;
    if (p.far == 0) {
        R->flight_time = r * A.time_step;
        R->finished = 1;
        __hip_atomic_fetch_sub(A.unfinished, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- the flight log (include/lscqp.h, "the flight log"): every replan's sampled states, flags and obstacle entries, kept per mission ----
//   MultiSyncSimulator::saveSimulationResultAsCSV   reference src/multi_sync_simulator.cpp:586-656 (what the rows become)
// Enqueued IN FRONT of record_kernel on the same stream: it reads the replan counter the record is about to increment, so row r holds
// replan r, and stream order is all the synchronisation there is.  A thread owns one (agent, sample) pair of mission blockIdx.x and
// stores to that pair's slots alone; no LDS, no atomics, no barrier.
struct LogArgs {
    int capacity, n_dyn;  // rows per mission, obstacle columns
    float* states;        // mission k at capacity * off[k] * S * 9: [capacity][n_k][S][9]
    int32_t* flags;       // mission k at capacity * off[k]:         [capacity][n_k]
    float* obstacles;     // [K][capacity][n_dyn][4]
    const lscqp_obstacle* table;  // [n_dyn] or NULL: no obstacle entries are written
};

__global__ __launch_bounds__(kThreads) void flight_log_kernel(Args A, LogArgs L) {
    const int k = blockIdx.x;
    const lscqp_mission_record* R = A.rec + k;
    if (R->finished != 0) return;  // frozen, as the record (the whole workgroup: one word, the same for every lane)
    const int r = R->replans;
    if (r >= L.capacity) return;  // full: the record goes on counting, lscqp_record_log_rows tells
    const int64_t lo = A.off ? A.off[k] : 0, hi = A.off ? A.off[k + 1] : A.n_total;
    const size_t n_k = (size_t)(hi - lo), S = (size_t)A.n_samples, cap = (size_t)L.capacity;
    if (blockIdx.y == 0 && L.table)
        for (int oi = threadIdx.x; oi < L.n_dyn; oi += kThreads) {
            const lscqp_obstacle* O = L.table + oi;
            float* o = L.obstacles + (((size_t)k * cap + (size_t)r) * (size_t)L.n_dyn + (size_t)oi) * 4;
            o[0] = (float)O->position[0], o[1] = (float)O->position[1], o[2] = (float)O->position[2], o[3] = (float)O->radius;
        }
    const size_t i = (size_t)blockIdx.y * kThreads + threadIdx.x;  // (agent, sample) of the mission
    if (i >= n_k * S) return;
    const size_t al = i / S, s = i - al * S;
    const int64_t a = lo + (int64_t)al;
    float pos[3], vel[3], acc[3];
    lscpost::state_at(A.M, A.dim, A.dt, (int)s * A.record_time_step, A.z_2d, A.x_all + a * (A.dim * 6 * A.M), pos, vel, acc);
    float* o = L.states + cap * (size_t)lo * S * 9 + (((size_t)r * n_k + al) * S + s) * 9;
    o[0] = pos[0], o[1] = pos[1], o[2] = pos[2];
    o[3] = vel[0], o[4] = vel[1], o[5] = vel[2];
    o[6] = acc[0], o[7] = acc[1], o[8] = acc[2];
    if (s == 0) {  // the five per-agent conditions the record counts
        int w = A.status[a] != LSCQP_STATUS_OPTIMAL ? LSCQP_LOG_FLAG_QP_FAILED : 0;
        w |= A.valid[a] == 0 ? LSCQP_LOG_FLAG_INVALID : 0;
        w |= A.goal_status[a] != 0 ? LSCQP_LOG_FLAG_GOAL_FAILED : 0;
        w |= A.sfc_status[a] == 0 ? LSCQP_LOG_FLAG_SFC_KEPT : 0;
        w |= (A.waypoint_updated && A.waypoint_updated[a] != 0) ? LSCQP_LOG_FLAG_WAYPOINT : 0;
        L.flags[cap * (size_t)lo + (size_t)r * n_k + al] = w;
    }
}

// ---- the obstacle record (include/lscqp.h, "the obstacle record"): each mission's least agent-obstacle safety ratio over the flight ----
//   MultiSyncSimulator::update   reference src/multi_sync_simulator.cpp:527-557 (`if (safety_ratio_obs > current)`), written at :658-709
// Enqueued IN FRONT of flight_log_kernel and record_kernel on the same stream, for the same reason as the log: it reads the replan counter
// the record is about to increment and the `finished` word the record is about to set.  One workgroup per mission; a lane owns the
// entries of the agents it strides over, thread 0 the mission's slot.  No atomics, nothing the other two kernels read or write is written.
struct ObsArgs {
    int64_t n_total;
    const int64_t* off;  // as Args::off
    const lscqp_mission_record* rec;
    const lscqp_safety_obs* figures;          // [n_total], the replan's (borrowed)
    lscqp_mission_obstacle_record* missions;  // [K]
    lscqp_agent_obstacle_record* agents;      // [n_total]
};

struct ObsPart {
    double ratio;                 // least ratio of the replan, +inf: none
    int agent, obstacle, sample;  // ... the agent attaining it (lowest id on ties), its obstacle and sample; -1
    int compared, below_one;
};

// (ids compare as unsigned, as in `combine` above: -1, "none", loses every tie; a NaN is neither smaller nor equal and is never taken)
__device__ __forceinline__ void combine_obs(ObsPart& a, const ObsPart& b) {
    if (b.ratio < a.ratio || (b.ratio == a.ratio && (unsigned)b.agent < (unsigned)a.agent)) {
        a.ratio = b.ratio;
        a.agent = b.agent;
        a.obstacle = b.obstacle;
        a.sample = b.sample;
    }
    a.compared += b.compared;
    a.below_one += b.below_one;
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ void dpp_step_obs(ObsPart& p) {
    ObsPart q;
    q.ratio = dpp_f64<CTRL, ROW_MASK>(INFINITY, p.ratio);
    q.agent = dpp_i32<CTRL, ROW_MASK>(-1, p.agent);
    q.obstacle = dpp_i32<CTRL, ROW_MASK>(-1, p.obstacle);
    q.sample = dpp_i32<CTRL, ROW_MASK>(-1, p.sample);
    q.compared = dpp_i32<CTRL, ROW_MASK>(0, p.compared);
    q.below_one = dpp_i32<CTRL, ROW_MASK>(0, p.below_one);
    combine_obs(p, q);
}

__global__ __launch_bounds__(kThreads) void record_obstacles_kernel(ObsArgs A) {
    __shared__ ObsPart s_part[kWaves];
    const int k = blockIdx.x;
    const lscqp_mission_record* R = A.rec + k;
    if (R->finished != 0) return;  // frozen, as the record (the whole workgroup: one word, the same for every lane)
    const int r = R->replans;      // this replan's index: the record's kernel, behind this one, increments it
    const int64_t lo = A.off ? A.off[k] : 0, hi = A.off ? A.off[k + 1] : A.n_total;
    ObsPart p = {INFINITY, -1, -1, -1, 0, 0};
    for (int64_t a = lo + threadIdx.x; a < hi; a += kThreads) {
        const lscqp_safety_obs* S = A.figures + a;
        const double v = S->safety_ratio_obs;
        lscqp_agent_obstacle_record* E = A.agents + a;
        if (v < E->safety_ratio_obs) {  // strict <: an earlier replan keeps a tie, a NaN is never taken
            E->safety_ratio_obs = v;
            E->replan = r, E->obstacle = S->closest_obstacle, E->sample = S->sample;
        }
        // (ascending ids within a lane: the strict < of combine_obs keeps the lowest)
        const ObsPart q = {v, (int)a, S->closest_obstacle, S->sample, fabs(v) < INFINITY ? 1 : 0, v < 1.0 ? 1 : 0};
        combine_obs(p, q);
    }
    dpp_step_obs<0x111, 0xf>(p);  // (the steps of wave_reduce: lane 63 ends up with the wavefront's figures)
    dpp_step_obs<0x112, 0xf>(p);
    dpp_step_obs<0x114, 0xf>(p);
    dpp_step_obs<0x118, 0xf>(p);
    dpp_step_obs<0x142, 0xa>(p);
    dpp_step_obs<0x143, 0xc>(p);
    if ((threadIdx.x & 63) == 63) s_part[threadIdx.x >> 6] = p;
    __syncthreads();
    if (threadIdx.x != 0) return;
    p = s_part[0];
    for (int w = 1; w < kWaves; w++) combine_obs(p, s_part[w]);
    lscqp_mission_obstacle_record* O = A.missions + k;
    if (p.ratio < O->safety_ratio_obs) {  // strict <: the reference's `if (safety_ratio_obs > current)`, replan after replan
        O->safety_ratio_obs = p.ratio;
        O->replan = r, O->agent = p.agent, O->obstacle = p.obstacle, O->sample = p.sample;
    }
    O->below_one += p.below_one;
    O->compared += p.compared;
}

}  // namespace lscrecord

struct lscqp_record_s {
    lscrecord::Args a;  // (the per-step pointers are filled by lscqp_record_step_device)
    int K = 1;
    int device = 0;
    // the flight log (lscqp_record_set_log): capacity = 0 = none, the record enqueues what it always did
    struct Log {
        int32_t capacity = 0, n_dyn = 0;
        unsigned tiles = 1;  // workgroups per mission: the largest mission's (agent, sample) pairs in tiles of kThreads
        lscqp::dev_ptr<float> states, obstacles;
        lscqp::dev_ptr<int32_t> flags;
        const lscqp_obstacle* table = nullptr;  // borrowed (lscqp_record_log_obstacles)
    } log;
    // the obstacle record (lscqp_record_set_obstacle_figures): figures = NULL = none, the record enqueues what it always did.  ONE side
    // allocation in the layout of include/lscqp.h (lscqp_record_obstacles_raw): spare | missions [K] | spare | agents [n_total] | spare
    struct Obstacles {
        const lscqp_safety_obs* figures = nullptr;  // borrowed
        lscqp::dev_ptr<unsigned char> side;
    } obs;
    size_t obs_missions_at() const { return LSCQP_OBSREC_SPARE; }
    size_t obs_agents_at() const { return 2 * (size_t)LSCQP_OBSREC_SPARE + (size_t)K * sizeof(lscqp_mission_obstacle_record); }
    size_t obs_bytes() const { return obs_agents_at() + (size_t)a.n_total * sizeof(lscqp_agent_obstacle_record) + LSCQP_OBSREC_SPARE; }
    std::vector<int64_t> off;        // [K + 1]
    lscqp::dev_ptr<int64_t> d_off;   // own copy of the offsets, or empty where the caller's device copy is borrowed
    lscqp::dev_ptr<float> goal, points, last;
    lscqp::dev_ptr<double> dist;
    lscqp::dev_ptr<lscqp_mission_record> rec;
    lscqp::dev_ptr<int32_t> unfinished;
    lscqp::pinned_ptr<int32_t> h_word;  // pinned: where lscqp_plan_run's 4-byte copies land
};

using lscqp::hip_fail;
using lscqp::OnDevice;

// the obstacle record's cleared state -- +inf, -1, 0 -- copied into `side` (the spare bytes around the two arrays are not written); synchronous
static hipError_t clear_obstacle_record(const lscqp_record_s* r, unsigned char* side) {
    std::vector<lscqp_mission_obstacle_record> ms((size_t)r->K);
    for (lscqp_mission_obstacle_record& m : ms) {
        m.safety_ratio_obs = INFINITY;
        m.replan = m.agent = m.obstacle = m.sample = -1;
        m.below_one = m.compared = 0;
    }
    std::vector<lscqp_agent_obstacle_record> as((size_t)r->a.n_total);
    for (lscqp_agent_obstacle_record& e : as) {
        e.safety_ratio_obs = INFINITY;
        e.replan = e.obstacle = e.sample = -1;
        e.reserved = 0;
    }
    hipError_t e = hipMemcpy(side + r->obs_missions_at(), ms.data(), ms.size() * sizeof ms[0], hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(side + r->obs_agents_at(), as.data(), as.size() * sizeof as[0], hipMemcpyHostToDevice);
    return e;
}

extern "C" int lscqp_record_create_(lscqp_handle h, int64_t n_total, int32_t n_missions, const int64_t* mission_offsets,
                                    const int64_t* d_offsets_borrowed, int32_t n_samples, double record_time_step, double time_step, double z_2d,
                                    const lscqp_record_desc* desc, lscqp_record* out) {
    if (!h || !desc || !out) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null argument");
    if (n_total <= 0 || n_total > 0x7fffffff) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_record_create: 0 < n_total < 2^31 required");
    if (n_samples <= 0 || !(record_time_step > 0) || !(time_step > 0))
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_record_create: n_samples > 0, record_time_step > 0 and time_step > 0 required");
    if (!(desc->goal_threshold >= 0)) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_record_create: goal_threshold must be >= 0");
    const bool single = !mission_offsets;
    if (!single) {
        const int rc = lscqp_check_missions_(n_total, n_missions, mission_offsets);
        if (rc != LSCQP_OK) return rc;
    }
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return lscqp_set_error_(LSCQP_ERR_NO_DEVICE, "no HIP device: lscqp has no CPU fallback");
    std::unique_ptr<lscqp_record_s> r(new lscqp_record_s());
    memset(&r->a, 0, sizeof r->a);
    r->device = dev;
    r->K = single ? 1 : n_missions;
    if (single) r->off = {0, n_total};
    else r->off.assign(mission_offsets, mission_offsets + n_missions + 1);
    const lscqp_class_desc* cd = lscqp_class_desc_of_(h);
    const int M = lscqp_num_segments(h);
    r->a.M = M, r->a.dim = lscqp_num_variables(h) / (6 * M), r->a.n_samples = n_samples;
    r->a.dt = cd->dt, r->a.record_time_step = record_time_step, r->a.time_step = time_step, r->a.z_2d = z_2d;
    r->a.goal_threshold = desc->goal_threshold;
    r->a.n_total = n_total;
    const size_t nt = (size_t)n_total;
    const char* const what = "lscqp_record_create";
    if (!single && !d_offsets_borrowed) {
        if (const int rc = lscqp::dev_alloc(r->d_off, (size_t)n_missions + 1, what)) return rc;
        const hipError_t e = hipMemcpy(r->d_off.get(), mission_offsets, (size_t)(n_missions + 1) * sizeof(int64_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_fail(e, what);
    }
    if (const int rc = lscqp::dev_alloc(r->goal, nt * 3, what)) return rc;
    if (const int rc = lscqp::dev_alloc(r->points, nt * (size_t)n_samples * 3, what)) return rc;
    if (const int rc = lscqp::dev_alloc(r->last, nt * 3, what)) return rc;
    if (const int rc = lscqp::dev_alloc(r->dist, nt, what)) return rc;
    if (const int rc = lscqp::dev_alloc(r->rec, (size_t)r->K, what)) return rc;
    if (const int rc = lscqp::dev_alloc(r->unfinished, 1, what)) return rc;
    {
        void* word = nullptr;
        const hipError_t e = hipHostMalloc(&word, sizeof(int32_t), hipHostMallocDefault);
        if (e != hipSuccess) return hip_fail(e, what);
        r->h_word.reset((int32_t*)word);
    }
    r->a.off = single ? nullptr : (d_offsets_borrowed ? d_offsets_borrowed : r->d_off.get());
    r->a.goal = r->goal.get(), r->a.points = r->points.get(), r->a.last = r->last.get(), r->a.dist = r->dist.get(), r->a.rec = r->rec.get();
    r->a.unfinished = r->unfinished.get();
    std::vector<double> zero(nt * 3, 0.0);
    if (const int rc = lscqp_record_reset(r.get(), zero.data())) return rc;
    *out = r.release();
    return LSCQP_OK;
}

extern "C" {

int lscqp_record_create(lscqp_handle h, int64_t n_total, int32_t n_missions, const int64_t* mission_offsets, int32_t n_samples,
                        double record_time_step, double time_step, double z_2d, const lscqp_record_desc* desc, lscqp_record* out) {
    return lscqp_record_create_(h, n_total, n_missions, mission_offsets, nullptr, n_samples, record_time_step, time_step, z_2d, desc, out);
}

void lscqp_record_destroy(lscqp_record r) {
    if (!r) return;
    OnDevice on(r->device);
    (void)hipDeviceSynchronize();
    delete r;
}

int lscqp_record_reset(lscqp_record r, const double* goal_points) {
    if (!r || !goal_points) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null argument");
    OnDevice on(r->device);
    const size_t nt = (size_t)r->a.n_total;
    std::vector<float> gl(nt * 3);
    for (size_t i = 0; i < nt * 3; i++) gl[i] = (float)goal_points[i];
    std::vector<lscqp_mission_record> rec((size_t)r->K);
    for (lscqp_mission_record& m : rec) {
        memset(&m, 0, sizeof m);
        m.first_qp_failed_replan = -1;
        m.flight_time = -1.0;
        m.safety_ratio_agent = INFINITY;
        m.safety_replan = m.safety_agent = m.safety_other = -1;
    }
    const int32_t K = r->K;
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(r->goal.get(), gl.data(), gl.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(r->rec.get(), rec.data(), rec.size() * sizeof(lscqp_mission_record), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(r->unfinished.get(), &K, sizeof K, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(r->dist.get(), 0, nt * sizeof(double));
    if (e == hipSuccess) e = hipMemset(r->last.get(), 0, nt * 3 * sizeof(float));
    if (e == hipSuccess) e = hipMemset(r->points.get(), 0, nt * (size_t)r->a.n_samples * 3 * sizeof(float));
    if (e == hipSuccess && r->obs.side) e = clear_obstacle_record(r, r->obs.side.get());
    return e == hipSuccess ? LSCQP_OK : hip_fail(e, "lscqp_record_reset");
}

int lscqp_record_step_device(lscqp_record r, const lscqp_header* d_hdr, const double* d_x_all, const int32_t* d_status, const int32_t* d_goal_status,
                             const int32_t* d_sfc_status, const int32_t* d_valid, const int32_t* d_in_range, const lscqp_safety* d_safety,
                             const int32_t* d_waypoint_updated, void* stream) {
    if (!r) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null record");
    if (!d_hdr || !d_x_all || !d_status || !d_goal_status || !d_sfc_status || !d_valid || !d_in_range || !d_safety)
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_record_step_device: null buffer (only d_waypoint_updated may be NULL)");
    lscrecord::Args a = r->a;
    a.hdr = d_hdr, a.x_all = d_x_all, a.status = d_status, a.goal_status = d_goal_status, a.sfc_status = d_sfc_status, a.valid = d_valid;
    a.in_range = d_in_range, a.safety = d_safety, a.waypoint_updated = d_waypoint_updated;
    if (r->obs.figures) {  // in front of the log and the record: the replan's obstacle figures of every mission still flying
        unsigned char* const side = r->obs.side.get();
        const lscrecord::ObsArgs o = {a.n_total, a.off, a.rec, r->obs.figures, (lscqp_mission_obstacle_record*)(side + r->obs_missions_at()),
                                      (lscqp_agent_obstacle_record*)(side + r->obs_agents_at())};
        hipLaunchKernelGGL(lscrecord::record_obstacles_kernel, dim3((unsigned)r->K), dim3(lscrecord::kThreads), 0, (hipStream_t)stream, o);
    }
    if (r->log.capacity > 0) {  // in front of the record: row `replans` of every mission still flying
        const lscqp_record_s::Log& g = r->log;
        const lscrecord::LogArgs l = {g.capacity, g.n_dyn, g.states.get(), g.flags.get(), g.obstacles.get(), g.table};
        hipLaunchKernelGGL(lscrecord::flight_log_kernel, dim3((unsigned)r->K, g.tiles), dim3(lscrecord::kThreads), 0, (hipStream_t)stream, a, l);
    }
    hipLaunchKernelGGL(lscrecord::record_kernel, dim3((unsigned)r->K), dim3(lscrecord::kThreads), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "HIP launch failed (mission record)");
    return LSCQP_OK;
}

int lscqp_record_download(lscqp_record r, lscqp_mission_record* out, double* agent_distance) {
    if (!r || !out) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null argument");
    OnDevice on(r->device);
    std::vector<double> dist((size_t)r->a.n_total);
    hipError_t e = hipMemcpy(out, r->rec.get(), (size_t)r->K * sizeof(lscqp_mission_record), hipMemcpyDeviceToHost);  // waits for the device
    if (e == hipSuccess) e = hipMemcpy(dist.data(), r->dist.get(), dist.size() * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "lscqp_record_download");
    for (int k = 0; k < r->K; k++) {  // the agents' distances in id order
        double s = 0;
        for (int64_t a = r->off[k]; a < r->off[k + 1]; a++) s += dist[(size_t)a];
        out[k].distance = s;
    }
    if (agent_distance) memcpy(agent_distance, dist.data(), dist.size() * sizeof(double));
    return LSCQP_OK;
}

void* lscqp_record_points(lscqp_record r, uint64_t* bytes_out) {
    if (!r) {
        lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null record");
        return nullptr;
    }
    if (bytes_out) *bytes_out = (uint64_t)r->a.n_total * (uint64_t)r->a.n_samples * 3 * sizeof(float);
    return r->points.get();
}

int lscqp_record_unfinished(lscqp_record r, int32_t* unfinished_out) {
    if (!r || !unfinished_out) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null argument");
    OnDevice on(r->device);
    const hipError_t e = hipMemcpy(unfinished_out, r->unfinished.get(), sizeof(int32_t), hipMemcpyDeviceToHost);
    return e == hipSuccess ? LSCQP_OK : hip_fail(e, "lscqp_record_unfinished");
}

int lscqp_record_set_log(lscqp_record r, int32_t max_replans, int32_t n_dyn) {
    if (!r) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null record");
    if (max_replans < 0 || n_dyn < 0) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_record_set_log: max_replans >= 0 and n_dyn >= 0 required");
    const size_t nt = (size_t)r->a.n_total, S = (size_t)r->a.n_samples, C = (size_t)max_replans, K = (size_t)r->K;
    size_t pairs = 0;  // the largest mission's (agent, sample) pairs
    for (size_t k = 0; k < K; k++) pairs = std::max(pairs, (size_t)(r->off[k + 1] - r->off[k]) * S);
    const size_t tiles = std::max<size_t>(1, (pairs + lscrecord::kThreads - 1) / lscrecord::kThreads);
    // (sizes in size_t; the bounds keep every product below 2^63 and the grid's second dimension a legal one)
    if (tiles > 65535 || (double)C * (double)nt * (double)S * 36.0 > 0x1p46 || (double)K * (double)C * (double)n_dyn * 16.0 > 0x1p46)
        return lscqp_set_error_(LSCQP_ERR_UNSUPPORTED, "lscqp_record_set_log: a log of this size is not kept (64 TiB, or more than 65535 tiles of 256 samples in a mission)");
    OnDevice on(r->device);
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "lscqp_record_set_log");
    lscqp_record_s::Log next;  // (none: empty)
    if (max_replans > 0) {  // (everything that can fail comes before the record changes)
        const char* const what = "lscqp_record_set_log";
        if (const int rc = lscqp::dev_alloc(next.states, C * nt * S * 9, what, true)) return rc;
        if (const int rc = lscqp::dev_alloc(next.flags, C * nt, what, true)) return rc;
        if (const int rc = lscqp::dev_alloc(next.obstacles, std::max<size_t>(1, K * C * (size_t)n_dyn * 4), what, true)) return rc;
        next.capacity = max_replans, next.n_dyn = n_dyn, next.tiles = (unsigned)tiles;  // (no table: lscqp_record_log_obstacles names it)
    }
    r->log = std::move(next);
    return LSCQP_OK;
}

int lscqp_record_log_obstacles(lscqp_record r, const lscqp_obstacle* d_table) {
    if (!r) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null record");
    if (r->log.capacity == 0) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_record_log_obstacles: the record has no log (lscqp_record_set_log)");
    if (d_table && r->log.n_dyn == 0)
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_record_log_obstacles: the log has no obstacle columns (n_dyn = 0 at lscqp_record_set_log)");
    r->log.table = d_table;
    return LSCQP_OK;
}

void* lscqp_record_log(lscqp_record r, int32_t which, uint64_t* bytes_out) {
    if (bytes_out) *bytes_out = 0;
    if (!r || r->log.capacity == 0 || which < 0 || which >= LSCQP_LOG_COUNT) {
        lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, !r ? "null record" : r->log.capacity == 0 ? "lscqp_record_log: the record has no log (lscqp_record_set_log)" : "unknown log buffer");
        return nullptr;
    }
    const lscqp_record_s::Log& g = r->log;
    const uint64_t C = (uint64_t)g.capacity, nt = (uint64_t)r->a.n_total, S = (uint64_t)r->a.n_samples;
    switch (which) {
    case LSCQP_LOG_STATES:
        if (bytes_out) *bytes_out = C * nt * S * 9 * sizeof(float);
        return g.states.get();
    case LSCQP_LOG_FLAGS:
        if (bytes_out) *bytes_out = C * nt * sizeof(int32_t);
        return g.flags.get();
    default:
        if (bytes_out) *bytes_out = (uint64_t)r->K * C * (uint64_t)g.n_dyn * 4 * sizeof(float);
        return g.obstacles.get();
    }
}

int lscqp_record_log_rows(lscqp_record r, int32_t* rows, int32_t* overflowed) {
    if (!r || !rows) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null argument");
    if (r->log.capacity == 0) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_record_log_rows: the record has no log (lscqp_record_set_log)");
    OnDevice on(r->device);
    std::vector<lscqp_mission_record> rec((size_t)r->K);
    const hipError_t e = hipMemcpy(rec.data(), r->rec.get(), rec.size() * sizeof(lscqp_mission_record), hipMemcpyDeviceToHost);  // waits for the device
    if (e != hipSuccess) return hip_fail(e, "lscqp_record_log_rows");
    for (int k = 0; k < r->K; k++) {
        rows[k] = std::min(rec[(size_t)k].replans, r->log.capacity);
        if (overflowed) overflowed[k] = rec[(size_t)k].replans > r->log.capacity;
    }
    return LSCQP_OK;
}

int lscqp_record_log_download(lscqp_record r, int32_t mission, int32_t first_replan, int32_t n_replans, float* states, int32_t* flags, float* obstacles) {
    if (!r) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null record");
    const lscqp_record_s::Log& g = r->log;
    if (g.capacity == 0) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_record_log_download: the record has no log (lscqp_record_set_log)");
    if (mission < 0 || mission >= r->K || first_replan < 0 || n_replans < 0)
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_record_log_download: 0 <= mission < n_missions, first_replan >= 0 and n_replans >= 0 required");
    OnDevice on(r->device);
    lscqp_mission_record m;
    hipError_t e = hipMemcpy(&m, r->rec.get() + mission, sizeof m, hipMemcpyDeviceToHost);  // waits for the device
    if (e != hipSuccess) return hip_fail(e, "lscqp_record_log_download");
    const int64_t rows = std::min(m.replans, g.capacity);
    if ((int64_t)first_replan + n_replans > rows)
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, ("lscqp_record_log_download: replans [" + std::to_string(first_replan) + ", " +
                                                             std::to_string((int64_t)first_replan + n_replans) + ") exceed the mission's " +
                                                             std::to_string(rows) + " logged rows").c_str());
    if (n_replans == 0) return LSCQP_OK;
    const size_t lo = (size_t)r->off[(size_t)mission], n_k = (size_t)r->off[(size_t)mission + 1] - lo, S = (size_t)r->a.n_samples, C = (size_t)g.capacity;
    const size_t f = (size_t)first_replan, n = (size_t)n_replans, nd = (size_t)g.n_dyn;
    if (states) e = hipMemcpy(states, g.states.get() + C * lo * S * 9 + f * n_k * S * 9, n * n_k * S * 9 * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess && flags) e = hipMemcpy(flags, g.flags.get() + C * lo + f * n_k, n * n_k * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && obstacles && nd > 0)
        e = hipMemcpy(obstacles, g.obstacles.get() + (((size_t)mission * C + f) * nd) * 4, n * nd * 4 * sizeof(float), hipMemcpyDeviceToHost);
    return e == hipSuccess ? LSCQP_OK : hip_fail(e, "lscqp_record_log_download");
}

int lscqp_record_set_obstacle_figures(lscqp_record r, const lscqp_safety_obs* d_safety_obs) {
    if (!r) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null record");
    OnDevice on(r->device);
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "lscqp_record_set_obstacle_figures");
    if (!d_safety_obs) {
        r->obs = {};
        return LSCQP_OK;
    }
    if (!r->obs.side) {  // first use: the side allocation, cleared (everything that can fail comes before the record changes)
        lscqp::dev_ptr<unsigned char> side;
        if (const int rc = lscqp::dev_alloc(side, r->obs_bytes(), "lscqp_record_set_obstacle_figures", true)) return rc;
        if ((e = clear_obstacle_record(r, side.get())) != hipSuccess) return hip_fail(e, "lscqp_record_set_obstacle_figures");
        r->obs.side = std::move(side);
    }
    r->obs.figures = d_safety_obs;
    return LSCQP_OK;
}

int lscqp_record_obstacles_download(lscqp_record r, lscqp_mission_obstacle_record* out, lscqp_agent_obstacle_record* agents) {
    if (!r || !out) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null argument");
    if (!r->obs.side)
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_record_obstacles_download: the record keeps no obstacle figures (lscqp_record_set_obstacle_figures)");
    OnDevice on(r->device);
    const unsigned char* const side = r->obs.side.get();
    hipError_t e = hipMemcpy(out, side + r->obs_missions_at(), (size_t)r->K * sizeof *out, hipMemcpyDeviceToHost);  // waits for the device
    if (e == hipSuccess && agents) e = hipMemcpy(agents, side + r->obs_agents_at(), (size_t)r->a.n_total * sizeof *agents, hipMemcpyDeviceToHost);
    return e == hipSuccess ? LSCQP_OK : hip_fail(e, "lscqp_record_obstacles_download");
}

void* lscqp_record_obstacles_raw(lscqp_record r, uint64_t* bytes_out) {
    if (bytes_out) *bytes_out = 0;
    if (!r || !r->obs.side) {
        lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, !r ? "null record" : "lscqp_record_obstacles_raw: the record keeps no obstacle figures (lscqp_record_set_obstacle_figures)");
        return nullptr;
    }
    if (bytes_out) *bytes_out = (uint64_t)r->obs_bytes();
    return r->obs.side.get();
}

int lscqp_record_unfinished_on_(lscqp_record r, void* stream, int32_t* unfinished_out) {
    hipError_t e = hipMemcpyAsync(r->h_word.get(), r->unfinished.get(), sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "lscqp_plan_run");
    *unfinished_out = *r->h_word;
    return LSCQP_OK;
}

}  // extern "C"
