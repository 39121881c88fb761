// lscplan.hip — one replan of a whole batch of agents as ONE chain of device work, gfx950 only: the device analogue of
//   TrajPlanner::plan / planImpl          reference src/traj_planner.cpp:33-60, 117-139
//   MultiSyncSimulator's per-agent loop   src/multi_sync_simulator.cpp:305-352 (who is whose obstacle), :354-400 (plan, doStep)
// planImpl's steps map onto the kernels of this library, all enqueued on one stream without a host round trip:
//   obstaclePrediction + initialTrajPlanning (PrevSol)  -> lscqp_shift_traj(_partial)_device over every agent's previous plan
//   broadcastMsgs' range filter                         -> lscqp_select_neighbours_device
//   constructLSC                                        -> lscqp_generate_constraints_device (LSC / CLSC / BVC)
//   constructSFC                                        -> lscqp_construct_sfc_device (initializeSFC on the first replan)
//   goalPlanning (grid-based planner goal mode)         -> lscqp_optimize_goal_device, result held as point3d (float32)
//   trajOptimization + failsafe (:755-803)              -> lscqp_solve_batch_device_ex (+ device-side second pass), failed QPs
//                                                          keep the initial trajectory
//   prev_traj = desired_traj; AgentManager::doStep      -> the plan buffer is updated in place; lscqp_validate_step_device
// Two small kernels of this file glue them: `prepare` (headers, corridor seed points, the initial trajectory in the solver's
// layout) and `commit` (failsafe, goal point).  Because nothing in the chain synchronises, allocates or copies through the
// host, the whole replan can be captured once in a hipGraph and replayed (lscqp_plan_step_graph): one graph launch instead of
// ten kernel launches per replan.  The waypoints of the grid planner / MAPF layer are either written into the plan's waypoint buffer by
// the caller before each step (waypoint_mode 0) or decided at the head of the chain by lscqp_waypoints_device (waypoint_mode 1, lscgrid.hip):
//   MultiSyncSimulator::decentralizedMAPP               -> lscqp_waypoints_device over the state, plans and goal points of the last replan
// A plan with a mission partition (lscqp_plan_set_missions) flies many independent missions in the same chain, over its one map: the three
// steps in which agents see each other -- the waypoint decision, the range filter, the safety figures -- run as their mission-aware twins,
// every other step is per agent and does not know.
// A plan whose missions have a world each (lscqp_plan_set_worlds: world k of a set of maps of one shape for mission k, as the reference's
// evaluation sets pair them) swaps two things and adds no node: its corridor node is the worlds launch, every agent tested against the map
// of its mission, and its grid starts each mission's occupancy from that world's base.
// A plan whose obstacles have drives (lscqp_plan_set_obstacle_drives: chasing and gaussian obstacles) gains one node more, obstacle_drive_kernel in
// front of the advance.
// A plan with dynamic obstacles (lscqp_plan_set_obstacles) gains three nodes: the obstacles' motion (lscobstacle.hip) in front of `prepare`, their
// rows (the non-agent branch of generateLSC or of generateCLSC, by the plan's constraint_mode; a BVC plan takes no obstacles) behind the agents'
// rows -- they take the first row slots of every agent -- and the obstacle leg of the safety figures behind the agents'.
// ObstacleGenerator::update(t, 0) -> obstacle_advance_kernel, src/multi_sync_simulator.cpp:311.
// A partition whose missions have obstacles of their own (lscqp_plan_set_mission_obstacles: one mission-major table, a clock per mission) has
// the same nodes in the same places, and the same kernels: the plan keeps its obstacles as T tables with a clock each and every agent's own list
// of table indices, one shared table being T = 1, and enqueues obstacle_advance_kernel<true>, obstacle_drive_kernel<true> over the T tables
// and the row entries over the lists; the safety leg is safety_obstacles_kernel<true> over the lists, <false> over the one table that is
// everybody's (enqueue_obstacle_safety).
// A plan that flies a patrol (lscqp_plan_set_patrol) gains the transition node directly behind the waypoint decision -- the reference decides the
// waypoints over the old goals, then every agent swaps start and goal on arrival at the top of its plan() -- and, with a grid, the node that
// exchanges the turned agents' distance fields behind it (lscpatrol.hip).
//   AgentManager::planningStateTransition (PATROL)      -> patrol_kernel, field_exchange_kernel
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/lscqp.h"
#include "lscqp_device.hpp"
#include "lscqp_internal.hpp"
// the obstacles' motion: obstacle_advance_kernel, lscqp_obstacle_model_prepare, lscqp_obstacles_advance_device (built as part of this unit)
#include "lscobstacle.hip"
// patrol missions: patrol_kernel, field_exchange_kernel and their entries (built as part of this unit)
#include "lscpatrol.hip"

namespace lscplan {

// A plan carries the work order of its QP launch from replan to replan when the launch exceeds what the chip works on at once
// (lscqp_launch_capacity: 256 instances of the M = 10 class, 1024 of M = 5), and that of its corridor launch from this many agents on
// (the throughput build of the corridor kernel keeps four agents per CU)
constexpr size_t kSfcOrderMin = 1024;
constexpr int kThreads = 64;
static_assert(kThreads == 64, "prepare_kernel hands data between the lanes of ONE wavefront (initial trajectory read before the prediction overwrites it)");

struct Shape {
    int M, dim, nv, n_obs;
    int64_t n_agents, n_total, first_agent;
    double z_2d, dt;
    int prediction_mode, initial_traj_mode;  // LSCQP_TRAJ_FROM_*
    double reset_threshold;                  // checkObstacleDisturbance, <= 0: off
};

// Trajectory::planConstVelTraj (src/trajectory.cpp:79-91): control point (m, i) = current_state + velocity * time in point3d (float)
// arithmetic, `time` a double that advances by segment_time / n after EVERY control point -- n + 1 steps per segment, so segment m
// starts at 1.2 m dt: the reference's own quirk, kept -- and is narrowed to float by Vector3::operator*(float).
__device__ __forceinline__ double const_vel_point(double p, double v, int idx, double dt) {
#pragma clang fp contract(off)
    double time = 0;
    for (int q = 0; q < idx; q++) time += dt / 5;
    const float step = (float)v * (float)time;
    return (double)((float)p + step);
}

// One wavefront per agent of the mission.  For every agent: its position (range filter) and its PREDICTED trajectory as the others'
// obstacle -- obstaclePrediction (src/traj_planner.cpp:228-253): the shifted previous plan that lscqp_shift_traj left in `traj`
// (PREVIOUSSOLUTION; constant velocity while planner_seq < 2, :276-279), or planConstVelTraj from the current state (POSITION /
// VELOCITY), then checkObstacleDisturbance (:312-319): a prediction that starts further than reset_threshold from where the agent is
// becomes "stays where it is".  For the local agents also: header, corridor seed points, and the INITIAL trajectory
// (initialTrajPlanning :360-423, same three sources but never reset: AgentManager's is_disturbed stays false) in the generator's layout
// (`own`) and in the solver's (`x_init`).  The initial trajectory is taken before the prediction overwrites the agent's entry of `traj`.
// x_shift != NULL: the agent's entry of `traj` is first made from the previous plans -- lscqp_shift_traj's whole-segment shift
// (lscgen.hip shift_traj_kernel: segment m := previous segment m + 1, the last one := the previous plan's last point, values rounded to
// float32, z := z_2d in the plane), one graph node less per replan.
__global__ __launch_bounds__(kThreads) void prepare_kernel(Shape s, int first_replan, const double* __restrict__ x_shift, const double* __restrict__ state,
                                                            const double* __restrict__ waypoint, const double* __restrict__ goal,
                                                            double* traj, const lscqp_agent_param* __restrict__ par,
                                                            double* __restrict__ pos, lscqp_header* __restrict__ hdr,
                                                            double* __restrict__ points, double* __restrict__ x_init, double* __restrict__ own) {
    const int64_t g = blockIdx.x;  // global agent id
    const int lane = threadIdx.x;
    if (g >= s.n_total) return;
    if (lane < 3) pos[g * 3 + lane] = state[g * 9 + lane];
    const int64_t t = g - s.first_agent;  // local id
    const bool local = t >= 0 && t < s.n_agents;
    double* tr = traj + g * s.M * 18;
    const int P18 = s.M * 18;
    if (x_shift != nullptr) {
        const double* x = x_shift + g * s.dim * s.M * 6;
        for (int e = lane; e < s.M * 6; e += kThreads) {
            const int m = e / 6, i = e - 6 * m;
            const int ms = (m + 1 < s.M) ? m + 1 : s.M - 1, is = (m + 1 < s.M) ? i : 5;
            double* o = tr + e * 3;
            o[0] = (double)(float)x[(0 * s.M + ms) * 6 + is];
            o[1] = (double)(float)x[(1 * s.M + ms) * 6 + is];
            o[2] = (s.dim == 3) ? (double)(float)x[(2 * s.M + ms) * 6 + is] : (double)(float)s.z_2d;
        }
        __syncthreads();  // (one wavefront per agent: its lanes read each other's entries below)
    }
    if (local) {
        const bool prev = s.initial_traj_mode == LSCQP_TRAJ_FROM_PREVIOUS_SOLUTION && !first_replan;
        const bool still = s.initial_traj_mode == LSCQP_TRAJ_FROM_POSITION;
        auto init_at = [&](int r, int k) -> double {  // control point r = 6 m + i, axis k
            return prev ? tr[r * 3 + k] : const_vel_point(state[g * 9 + k], still ? 0.0 : state[g * 9 + 3 + k], r, s.dt);
        };
        if (lane == 0) {
            lscqp_header H;
            memset(&H, 0, sizeof H);
            const lscqp_agent_param A = par[g];
            for (int k = 0; k < 3; k++) {
                H.p0[k] = state[g * 9 + k];
                H.v0[k] = state[g * 9 + 3 + k];
                H.a0[k] = state[g * 9 + 6 + k];
                H.goal[k] = goal[g * 3 + k];
                H.next_waypoint[k] = waypoint[t * 3 + k];
                H.vmax[k] = A.max_vel[k];
                H.amax[k] = A.max_acc[k];
            }
            H.radius = A.radius;
            H.nominal_velocity = A.nominal_velocity;
            H.n_obs = s.n_obs;
            H.terminal_segments = 0;  // set by finalize_goal_kernel once the goal LP has moved the goal
            hdr[t] = H;
        }
        if (lane < 9) {
            // generateSFC (src/traj_planner.cpp:738-753): the agent's position on the first replan, afterwards the hull
            // {initial_traj.lastPoint(), current_goal_point} and the next waypoint
            const int which = lane / 3, k = lane - 3 * which;
            const double p0k = state[g * 9 + k];
            const double v = which == 0 ? init_at((s.M - 1) * 6 + 5, k) : (which == 1 ? goal[g * 3 + k] : waypoint[t * 3 + k]);
            points[t * 9 + lane] = first_replan ? p0k : v;
        }
        double* xi = x_init + t * s.nv;
        for (int e = lane; e < s.nv; e += kThreads) {  // x_init[k][m][i] = initial_traj[m][i][k]
            const int k = e / (6 * s.M), r = e - k * 6 * s.M;
            xi[e] = init_at(r, k);
        }
        double* ow = own + t * P18;
        for (int e = lane; e < P18; e += kThreads) ow[e] = init_at(e / 3, e % 3);
    }
    // the agent as an obstacle of the others.  Every lane has finished reading tr[] (init_at above: x_init, own, the corridor seed
    // points) before any lane overwrites it with the prediction below.
    __syncthreads();
    const bool keep = s.prediction_mode == LSCQP_TRAJ_FROM_PREVIOUS_SOLUTION && !first_replan;
    bool reset = false;
    if (s.reset_threshold > 0) {
#pragma clang fp contract(off)
        // (startPoint() - position).norm(): float differences, float sum of squares, sqrt in double (octomath::Vector3)
        const float dx = (float)(keep ? tr[0] : state[g * 9 + 0]) - (float)state[g * 9 + 0];
        const float dy = (float)(keep ? tr[1] : state[g * 9 + 1]) - (float)state[g * 9 + 1];
        const float dz = (float)(keep ? tr[2] : state[g * 9 + 2]) - (float)state[g * 9 + 2];
        reset = sqrt((double)(dx * dx + dy * dy + dz * dz)) > s.reset_threshold;
    }
    if (!keep || reset) {
        const bool still = reset || s.prediction_mode == LSCQP_TRAJ_FROM_POSITION;
        for (int e = lane; e < P18; e += kThreads) {
            const int k = e % 3;
            tr[e] = const_vel_point(state[g * 9 + k], still ? 0.0 : state[g * 9 + 3 + k], e / 3, s.dt);
        }
    }
}

// after the goal LP: agent.current_goal_point is a point3d (GoalOptimizer::solve returns one, src/goal_optimizer.cpp:7-55), and
// getTerminalSegments_old (src/traj_optimizer.cpp:530-538) reads it with octomap's float32 vector arithmetic
__global__ __launch_bounds__(kThreads) void finalize_goal_kernel(Shape s, lscqp_header* __restrict__ hdr) {
#pragma clang fp contract(off)
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= s.n_agents) return;
    lscqp_header* H = hdr + t;
    float d[3];
    for (int k = 0; k < 3; k++) {
        const float gk = (float)H->goal[k];
        H->goal[k] = (double)gk;
        d[k] = gk - (float)H->p0[k];
    }
    const float nsq = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    const double ideal_flight_time = sqrt((double)nsq) / H->nominal_velocity;
    int ts = (int)((s.M * s.dt - ideal_flight_time + 1e-9) / s.dt);
    H->terminal_segments = ts > 1 ? ts : 1;
}

// owners of the library's own objects a plan holds
struct GridDestroy {
    void operator()(lscqp_grid g) const { lscqp_grid_destroy(g); }
};
struct RecordDestroy {
    void operator()(lscqp_record r) const { lscqp_record_destroy(r); }
};
struct HandleDestroy {
    void operator()(lscqp_handle h) const { lscqp_destroy(h); }
};

// the setters whose change waits for lscqp_plan_reset, in the order in which a step names them: bit i of lscqp_plan_s::pending
enum : unsigned {
    kPendMissions = 1u << 0,
    kPendRecord = 1u << 1,
    kPendObstacles = 1u << 2,
    kPendWorlds = 1u << 3,
    kPendFlightLog = 1u << 4,
    kPendDrives = 1u << 5,
    kPendPatrol = 1u << 6,
    kPendObstacleRecord = 1u << 7,
    kPendMissionObstacles = 1u << 8
};
constexpr const char* kPendSetter[] = {"lscqp_plan_set_missions", "lscqp_plan_set_record", "lscqp_plan_set_obstacles", "lscqp_plan_set_worlds",
                                       "lscqp_plan_set_flight_log", "lscqp_plan_set_obstacle_drives", "lscqp_plan_set_patrol",
                                       "lscqp_plan_set_obstacle_record", "lscqp_plan_set_mission_obstacles"};

}  // namespace lscplan

using lscqp::dev_ptr;
using lscqp::hip_fail;
using lscqp::OnDevice;

// What the plan owns frees itself with the plan (lscqp_plan_destroy has made the plan's device current and waited for it).  The state of each
// option is a struct of its own: its setter builds the new state complete in a local and moves it in, so a setter that fails changes nothing.
struct lscqp_plan_s {
    lscqp_handle hq = nullptr;  // the handle the QP solves run on: the caller's, or a private clone of its class in LSCQP_WARM_TIGHT mode
    std::unique_ptr<lscqp_solver, lscplan::HandleDestroy> own_hq;  // the clone, where hq is one
    lscqp_handle h = nullptr;
    lscqp_map map = nullptr;
    lscqp_plan_desc d;
    lscplan::Shape s;
    int device = 0;
    bool first = true;
    int64_t steps = 0;
    void* buf[LSCQP_PLAN_BUF_COUNT] = {};
    size_t bytes[LSCQP_PLAN_BUF_COUNT] = {};
    // private buffers
    lscqp_agent_param* par = nullptr;
    double *radius = nullptr, *downwash = nullptr, *traj = nullptr, *pos = nullptr, *points = nullptr, *x_init = nullptr, *x_new = nullptr, *own = nullptr;
    int32_t* nbr = nullptr;
    uint64_t* off = nullptr;
    int32_t* order = nullptr;  // work order of the next solve (only where the launch exceeds lscqp_launch_capacity)
    int32_t* sfc_order = nullptr;  // ... and of the next corridor launch, from the costs recorded by this one
    uint32_t* sfc_cost = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    hipStream_t cap = nullptr;
    // what the captured graph (and the tight-warm-start clone) was derived from: a later lscqp_update / lscqp_map_prepare bumps these
    uint64_t h_gen = 0, map_gen = 0;
    std::vector<dev_ptr<void>> owned;  // the buffers made at lscqp_plan_create, public and private
    // which setters changed the plan since the last lscqp_plan_reset (lscplan::kPend*): a step waits for the reset
    unsigned pending = 0;
    // waypoint_mode = LSCQP_WAYPOINT_GRID_PIBT: the grid, the mission's distance fields (one per agent, made by lscqp_plan_reset) and start points
    struct Waypoints {
        std::unique_ptr<lscqp_grid_s, lscplan::GridDestroy> grid;
        double resolution = 0.5, radius = 0;
        dev_ptr<int32_t> field;
        size_t field_nodes = 0;  // nodes per agent in `field`
        int32_t *init_d = nullptr, *desired_node = nullptr;  // (these three: made at lscqp_plan_create, in `owned`)
        double* start_pts = nullptr;
        bool fields_valid = false;
        int decision = LSCQP_DECISION_ONE_WORKGROUP;  // which form of the decision heads the chain (lscqp_plan_set_waypoint_decision)
    } wp;
    // a mission partition (lscqp_plan_set_missions): empty = one mission, the chain as it always was
    struct Missions {
        std::vector<int64_t> moff;  // [K + 1]
        dev_ptr<int64_t> d_moff;
    } mis;
    int n_missions() const { return mis.moff.empty() ? 1 : (int)mis.moff.size() - 1; }
    // a mission record (lscqp_plan_set_record): accumulated by the last node of the chain
    struct Record {
        bool on = false;
        lscqp_record_desc desc = {0.0};
        std::unique_ptr<lscqp_record_s, lscplan::RecordDestroy> held;  // of the partition in force; empty between set_missions and the reset
        int32_t log_capacity = 0;  // the flight log's rows per mission (lscqp_plan_set_flight_log), 0 = none: given to every record made
        bool obstacle_figures = false;  // the obstacle record (lscqp_plan_set_obstacle_record): every record made reads obs.safety
    } rec;
    // dynamic obstacles (lscqp_plan_set_obstacles, lscqp_plan_set_mission_obstacles): n_dyn = 0 = none, the chain as it always was.  The table
    // holds T tables one behind the other, table k the entries [ooff[k], ooff[k + 1]) with the clock word clock[k], n_dyn in all; the largest
    // one's count, n_slot, is the row slots [0, n_slot) the obstacles take of every agent, and ids [n_agents][n_slot] names every local
    // agent's entries by table index (-1: none).  One table shared by all agents is T = 1: offsets {0, n_dyn}, every agent's ids 0 .. n_dyn - 1
    struct Obstacles {
        int32_t n_dyn = 0, n_slot = 0, n_tables = 0;  // (n_tables: T, the tables and their clocks)
        lscqp_obstacle_param param = {};
        std::vector<lscqp_obstacle_model> models;  // prepared; HELD entries start at `start`
        dev_ptr<lscqp_obstacle_model> d_models;
        dev_ptr<lscqp_obstacle> table;
        dev_ptr<int32_t> ids, clock, d_ooff;
        dev_ptr<lscqp_safety_obs> safety;
        std::vector<int32_t> ooff;  // [T + 1]
        bool per_mission = false;   // table k belongs to mission k (lscqp_plan_set_mission_obstacles); else the one table is everybody's
        // the drives of chasing and gaussian obstacles (lscqp_plan_set_obstacle_drives): d_drives = NULL = none, the chain as it always was
        struct Drives {
            dev_ptr<lscqp_obstacle_drive> d_drives;
            dev_ptr<double> history;  // [n_history][3]
            int32_t n_history = 0;
            dev_ptr<lscqp_obstacle_drive_state> state;  // a checkpoint per obstacle
            std::vector<lscqp_obstacle_drive> host;      // (a table per mission only) the drives as they were given
        } drv;
    } obs;
    // a world per mission (lscqp_plan_set_worlds): set = NULL = the one map, the chain as it always was
    struct Worlds {
        lscqp_worlds set = nullptr;  // borrowed
        dev_ptr<int32_t> world_of;   // [n_total]: the agent's mission
        uint64_t gen = 0;            // the members' generation counters, summed, when the graph and the fields were derived
    } wld;
    // a patrol (lscqp_plan_set_patrol): on = false = none, the chain as it always was.  `desired` / `start` are the buffers the transition swaps:
    // the plan's own in grid mode (LSCQP_PLAN_BUF_DESIRED_GOAL, wp.start_pts) and LSCQP_PLAN_BUF_GOAL for static goals, else the patrol's
    struct Patrol {
        bool on = false;
        lscqp_patrol_desc desc = {0.0};
        double *desired = nullptr, *start = nullptr;
        dev_ptr<double> own_desired, own_start;
        dev_ptr<int32_t> legs, swapped;
        dev_ptr<int32_t> field_other, init_d_other;  // the opposite leg's fields (grid mode); the active ones are wp.field, wp.init_d
    } pat;
    bool wide() const { return wp.decision == LSCQP_DECISION_WIDE || (wp.decision == LSCQP_DECISION_AUTO && s.n_total >= LSCQP_DECISION_AUTO_MIN_AGENTS); }
};

namespace {

// a zeroed buffer of the plan's own, at least one element
template <class T>
int dalloc(lscqp_plan_s* p, T** out, size_t count) {
    dev_ptr<T> q;
    const size_t c = count ? count : 1;
    const int rc = lscqp::dev_alloc(q, c, "hipMalloc(plan buffer)");
    if (rc != LSCQP_OK) return rc;
    const hipError_t e = hipMemset(q.get(), 0, c * sizeof(T));
    if (e != hipSuccess) return hip_fail(e, "hipMemset(plan buffer)");
    *out = q.get();
    p->owned.emplace_back(q.release());
    return LSCQP_OK;
}

template <class T>
int dalloc_pub(lscqp_plan_s* p, int which, size_t count) {
    T* ptr = nullptr;
    const int rc = dalloc(p, &ptr, count);
    if (rc != LSCQP_OK) return rc;
    p->buf[which] = ptr;
    p->bytes[which] = count * sizeof(T);
    return LSCQP_OK;
}

#define PLAN_TRY(call)                 \
    do {                               \
        const int rc_ = (call);        \
        if (rc_ != LSCQP_OK) return rc_; \
    } while (0)

// The obstacle leg of the safety figures.  The by-ids entry over every agent's list serves every plan, bit for bit; the one table that is
// everybody's takes the whole-table instantiation of the same kernel text instead, here and nowhere else: with 250 agents its replan measured
// 3 to 4 us (1 %) more by ids, a list read per lane where the one table's addresses are uniform (NOTES.md section 46).  The motion's two nodes
// showed no such cost and take the per-mission entries over one table.
int enqueue_obstacle_safety(const lscqp_plan_s* p, const double* x_plan, hipStream_t stream) {
    const lscqp_plan_s::Obstacles& o = p->obs;
    const lscplan::Shape& s = p->s;
    if (!o.per_mission)
        return lscqp_safety_obstacles_device(p->h, s.n_agents, s.first_agent, s.n_total, p->d.safety_samples, p->d.record_time_step, s.z_2d, x_plan, p->radius,
                                             p->downwash, o.n_dyn, o.table.get(), o.safety.get(), stream);
    return lscqp_safety_obstacles_ids_device(p->h, s.n_agents, s.first_agent, s.n_total, p->d.safety_samples, p->d.record_time_step, s.z_2d, x_plan, p->radius,
                                             p->downwash, o.n_slot, o.ids.get(), o.n_dyn, o.table.get(), o.safety.get(), stream);
}

// the whole replan on `stream`; nothing here synchronises, allocates or touches host memory (capturable)
int enqueue(lscqp_plan_s* p, bool first_replan, hipStream_t stream) {
    const lscplan::Shape& s = p->s;
    if (s.n_agents == 0) return LSCQP_OK;  // an empty block of a sharded mission (9 agents over 4 devices: 3, 3, 3, 0): nothing to replan
    lscqp_handle h = p->h;
    double* state = (double*)p->buf[LSCQP_PLAN_BUF_STATE];
    double* waypoint = (double*)p->buf[LSCQP_PLAN_BUF_WAYPOINT];
    double* x_plan = (double*)p->buf[LSCQP_PLAN_BUF_PLAN];
    double* goal = (double*)p->buf[LSCQP_PLAN_BUF_GOAL];
    lscqp_header* hdr = (lscqp_header*)p->buf[LSCQP_PLAN_BUF_HEADER];
    lscqp_row* rows = (lscqp_row*)p->buf[LSCQP_PLAN_BUF_ROWS];
    lscqp_box* sfc = (lscqp_box*)p->buf[LSCQP_PLAN_BUF_SFC];
    int32_t* status = (int32_t*)p->buf[LSCQP_PLAN_BUF_STATUS];
    int32_t* goal_status = (int32_t*)p->buf[LSCQP_PLAN_BUF_GOAL_STATUS];
    int32_t* sfc_status = (int32_t*)p->buf[LSCQP_PLAN_BUF_SFC_STATUS];
    int32_t* valid = (int32_t*)p->buf[LSCQP_PLAN_BUF_VALID];
    int32_t* count = (int32_t*)p->buf[LSCQP_PLAN_BUF_IN_RANGE];
    double* state_out = (double*)p->buf[LSCQP_PLAN_BUF_NEXT_STATE];
    double* obj = (double*)p->buf[LSCQP_PLAN_BUF_OBJECTIVE];
    lscqp_info* info = (lscqp_info*)p->buf[LSCQP_PLAN_BUF_INFO];
    const double fraction = p->d.time_step / s.dt;
    const int K = p->n_missions();
    const lscqp_plan_s::Waypoints& wp = p->wp;
    const lscqp_plan_s::Obstacles& obs = p->obs;
    lscqp_grid grid = wp.grid.get();
    const int64_t *moff = p->mis.moff.data(), *d_moff = p->mis.d_moff.get();
    // row slots [0, n_slot): the obstacles, [n_slot, n_obs): the in-range agents (n_slot: the largest table's count, n_dyn of one table)
    const int32_t n_dyn = obs.n_dyn, n_slot = obs.n_slot, n_nbr = s.n_obs - n_slot;
    // decentralizedMAPP precedes the planning loop (src/multi_sync_simulator.cpp:101-120): the waypoints of this replan, from the plans as the
    // last replan left them (AgentManager::getTraj is desired_traj, un-shifted)
    if (grid) {
        if (K > 1)
            PLAN_TRY(lscqp_waypoints_missions_device(grid, lscqp_class_desc_of_(h)->communication_range, s.M, s.dim, s.n_total, K, moff, d_moff,
                                                     state, x_plan, goal, wp.field.get(), wp.init_d, waypoint, (int32_t*)p->buf[LSCQP_PLAN_BUF_GROUP], wp.desired_node,
                                                     (int32_t*)p->buf[LSCQP_PLAN_BUF_WAYPOINT_UPDATED], stream));
        else if (p->wide())
            PLAN_TRY(lscqp_waypoints_wide_device(grid, lscqp_class_desc_of_(h)->communication_range, s.M, s.dim, s.n_total, state, x_plan, goal, wp.field.get(), wp.init_d,
                                                 waypoint, (int32_t*)p->buf[LSCQP_PLAN_BUF_GROUP], wp.desired_node, (int32_t*)p->buf[LSCQP_PLAN_BUF_WAYPOINT_UPDATED], stream));
        else
            PLAN_TRY(lscqp_waypoints_device(grid, lscqp_class_desc_of_(h)->communication_range, s.M, s.dim, s.n_total, state, x_plan, goal, wp.field.get(), wp.init_d,
                                            waypoint, (int32_t*)p->buf[LSCQP_PLAN_BUF_GROUP], wp.desired_node, (int32_t*)p->buf[LSCQP_PLAN_BUF_WAYPOINT_UPDATED], stream));
    }
    // planningStateTransition's PATROL branch at the top of every agent's plan() (src/agent_manager.cpp:225-240): behind decentralizedMAPP, which
    // decided over the old goals, and in front of everything TrajPlanner::plan does.  An agent that turned flies by its other field from here on
    if (p->pat.on) {
        const lscqp_plan_s::Patrol& pat = p->pat;
        PLAN_TRY(lscqp_patrol_device(h, s.n_total, state, pat.desired, pat.start, pat.desc.goal_threshold, s.dim, s.z_2d, pat.legs.get(), pat.swapped.get(), stream));
        if (grid)
            PLAN_TRY(lscqp_field_exchange_device(s.n_total, (int64_t)wp.field_nodes, pat.swapped.get(), wp.field.get(), pat.field_other.get(), wp.init_d,
                                                 pat.init_d_other.get(), stream));
    }
    // obstacle_generator.update(t, 0) at the replan's start time (src/multi_sync_simulator.cpp:311); the clock is the device's.  Chasing and
    // gaussian obstacles first: they read the table as the last replan left it, and the agents' states of this replan's start
    // (one table is the entries' one-table case)
    if (n_dyn > 0 && obs.drv.d_drives)
        PLAN_TRY(lscqp_obstacles_drive_missions_device(h, obs.d_models.get(), obs.drv.d_drives.get(), obs.n_tables, obs.ooff.data(), obs.d_ooff.get(), n_dyn,
                                                       obs.drv.history.get(), obs.drv.n_history, state, s.n_total, obs.drv.state.get(), p->d.time_step,
                                                       obs.clock.get(), obs.table.get(), stream));
    if (n_dyn > 0)
        PLAN_TRY(lscqp_obstacles_advance_missions_device(h, obs.d_models.get(), obs.n_tables, obs.ooff.data(), obs.d_ooff.get(), n_dyn, p->d.time_step,
                                                         obs.clock.get(), obs.table.get(), stream));
    // obstaclePredictionWithPrevSol / initialTrajPlanningPrevSol for every agent of the mission (:273-310, 399-423)
    const bool from_plans = !first_replan && (s.prediction_mode == LSCQP_TRAJ_FROM_PREVIOUS_SOLUTION || s.initial_traj_mode == LSCQP_TRAJ_FROM_PREVIOUS_SOLUTION);
    const bool whole_shift = from_plans && fraction >= 1.0 - 1e-9;  // (done by prepare_kernel itself)
    if (from_plans && !whole_shift) PLAN_TRY(lscqp_shift_traj_partial_device(h, s.n_total, fraction, s.z_2d, x_plan, p->traj, stream));
    hipLaunchKernelGGL(lscplan::prepare_kernel, dim3((unsigned)s.n_total), dim3(lscplan::kThreads), 0, stream, s, first_replan ? 1 : 0,
                       whole_shift ? (const double*)x_plan : (const double*)nullptr, state, waypoint, goal, p->traj, p->par, p->pos, hdr, p->points, p->x_init, p->own);
    if (p->map) {
        // (large plans: most expensive corridor of the previous replan first, the costs of this one recorded for the next)
        const int32_t* sfc_order = nullptr;
        if (p->sfc_order && !first_replan) {
            PLAN_TRY(lscqp_order_by_cost_device(s.n_agents, p->sfc_cost, p->sfc_order, stream));
            sfc_order = p->sfc_order;
        }
        if (p->wld.set)  // every agent in the world of its mission (a partition has every agent local: first_agent = 0)
            PLAN_TRY(lscqp_construct_sfc_worlds_device(h, p->wld.set, first_replan ? LSCQP_SFC_INIT : p->d.sfc_mode, s.n_agents, p->wld.world_of.get(), p->points,
                                                       p->radius + s.first_agent, sfc, sfc_status, sfc_order, p->sfc_cost, stream));
        else
            PLAN_TRY(lscqp_construct_sfc_device_ordered(h, p->map, first_replan ? LSCQP_SFC_INIT : p->d.sfc_mode, s.n_agents, p->points,
                                                        p->radius + s.first_agent, sfc, sfc_status, sfc_order, p->sfc_cost, stream));
    }
    if (K > 1)
        PLAN_TRY(lscqp_select_neighbours_missions_device(h, s.n_total, K, moff, d_moff, n_nbr, lscqp_class_desc_of_(h)->communication_range, p->pos,
                                                         p->nbr, count, stream));
    else
        PLAN_TRY(lscqp_select_neighbours_device(h, s.n_agents, s.first_agent, s.n_total, n_nbr, lscqp_class_desc_of_(h)->communication_range, p->pos, p->nbr, count,
                                                stream));
    if (n_nbr > 0)
        PLAN_TRY(lscqp_generate_constraints_own_(h, p->d.constraint_mode, s.n_agents, n_nbr, s.first_agent, p->traj, p->own, p->nbr, p->radius,
                                                 p->downwash, goal, rows, s.n_obs, n_slot, stream));
    // the obstacles' rows (the non-agent branch of the plan's generator) over the planning agents' INITIAL trajectories: `own`, indexed by
    // local id like the radii, goals and headers handed over here -- `traj` holds the agents' predictions as each other's obstacles by now.
    // generateCLSC's rows take no obstacle goal points: Obstacle::goal_point is the origin in the reference (include/obstacle.hpp:23, 37-49)
    // (n_slot slots, the ids naming each agent's own entries -- a slot without one gets zero rows; only the LSC rows read the headers)
    if (n_dyn > 0)
        PLAN_TRY(lscqp_generate_obstacle_rows_device(h, p->d.constraint_mode, &obs.param, s.n_agents, n_slot, 0, p->own, obs.ids.get(), obs.table.get(), nullptr,
                                                     p->radius + s.first_agent, goal + s.first_agent * 3, hdr, rows, s.n_obs, 0, stream));
    if (p->d.optimize_goal) {  // (the goal LP's kernel finishes the headers itself: one node less)
        PLAN_TRY(lscqp_optimize_goal_fin_device_(h, s.n_agents, hdr, rows, p->off, p->map ? sfc : nullptr, goal_status, s.dt, stream));
    } else {
        const unsigned nb = (unsigned)((s.n_agents + lscplan::kThreads - 1) / lscplan::kThreads);
        hipLaunchKernelGGL(lscplan::finalize_goal_kernel, dim3(nb), dim3(lscplan::kThreads), 0, stream, s, hdr);
    }
    // Work order of the solve (include/lscqp.h): from the second replan on, the agents whose previous QP took the most iterations go
    // first -- the info records of the previous replan are still in place here.  Only where a launch can have a tail: more agents than
    // a few rounds of workgroups (below that every QP starts at once).
    const int32_t* order = nullptr;
    if (p->order && !first_replan) {
        PLAN_TRY(lscqp_order_by_work_device(s.n_agents, info, p->order, stream));
        order = p->order;
    }
    // retry = 3: the reference tries a failed QP again on the spot (src/traj_planner.cpp:763-766) -- here a second pass from the default start and
    // the RESCUE pass behind it are always enqueued (each returns per instance on OPTIMAL: two near-empty launches when nothing failed)
    PLAN_TRY(lscqp_solve_batch_device_ordered(p->hq, s.n_agents, s.n_obs, hdr, rows, p->off, p->map ? sfc : nullptr, p->x_init, p->x_new, obj,
                                              status, info, 3, order, stream));
    {   // commit (failsafe of trajOptimization, prev_traj = desired_traj, the goal point carried over) + isSolValid + doStep: one launch
        const lscqp_class_desc* cd = lscqp_class_desc_of_(h);
        if (cd->use_sfc && !p->map) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "the class has corridor rows but the plan has no map");
        PLAN_TRY(lscqp_commit_validate_raw_(s.M, s.dim, cd->use_sfc, s.dt, s.n_agents, p->d.time_step, s.z_2d, status, p->x_new, p->x_init,
                                            x_plan + s.first_agent * s.nv, goal + s.first_agent * 3, hdr, p->map ? sfc : nullptr, valid, state_out, stream));
    }
    if (p->d.safety_samples > 0 && K > 1)
        PLAN_TRY(lscqp_safety_metrics_missions_device(h, s.n_total, K, moff, d_moff, p->d.safety_samples, p->d.record_time_step, s.z_2d, x_plan,
                                                      p->radius, p->downwash, hdr, (lscqp_safety*)p->buf[LSCQP_PLAN_BUF_SAFETY], stream));
    else if (p->d.safety_samples > 0)  // MultiSyncSimulator::update's safety ratio / excess ratios over the step just planned (:486-577)
        PLAN_TRY(lscqp_safety_metrics_device(h, s.n_agents, s.first_agent, s.n_total, p->d.safety_samples, p->d.record_time_step, s.z_2d, x_plan,
                                             p->radius, p->downwash, hdr, (lscqp_safety*)p->buf[LSCQP_PLAN_BUF_SAFETY], stream));
    // the obstacle leg of the safety figures (:527-557), against the positions this replan's advance left
    if (p->d.safety_samples > 0 && n_dyn > 0) PLAN_TRY(enqueue_obstacle_safety(p, x_plan, stream));
    // the mission record: the figures of this replan and the finish test on the state it started from (hdr.p0), the chain's last node (a
    // record with a flight log enqueues the log's node in front of its own)
    if (p->rec.on)
        PLAN_TRY(lscqp_record_step_device(p->rec.held.get(), hdr, x_plan, status, goal_status, sfc_status, valid, count, (const lscqp_safety*)p->buf[LSCQP_PLAN_BUF_SAFETY],
                                          (const int32_t*)p->buf[LSCQP_PLAN_BUF_WAYPOINT_UPDATED], stream));
    // (closed loop: LSCQP_PLAN_BUF_NEXT_STATE is the local agents' slice of the state buffer itself, so doStep's result is the next
    // replan's current state without a copy)
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "HIP launch failed (plan step)");
    return LSCQP_OK;
}

void drop_graph(lscqp_plan_s* p) {
    if (p->exec) (void)hipGraphExecDestroy(p->exec);
    if (p->graph) (void)hipGraphDestroy(p->graph);
    p->exec = nullptr;
    p->graph = nullptr;
}

// may the plan step?  The refusals of a plan that waits for lscqp_plan_reset, in the order a step has always given them.  Asked before
// anything is enqueued or captured
int may_step(const lscqp_plan_s* p) {
    if (p->s.n_agents == 0) return LSCQP_OK;  // (an empty block of a sharded mission replans nothing)
    unsigned waits = p->pending;
    if (p->rec.on && !p->rec.held) waits |= lscplan::kPendRecord;
    for (unsigned i = 0; i < sizeof lscplan::kPendSetter / sizeof *lscplan::kPendSetter; i++)
        if (waits & (1u << i))
            return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, (std::string(lscplan::kPendSetter[i]) + ": lscqp_plan_reset must come before the next step").c_str());
    if (p->wp.grid && !p->wp.fields_valid)
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "waypoint_mode = LSCQP_WAYPOINT_GRID_PIBT: lscqp_plan_reset must come before the first step");
    return LSCQP_OK;
}

// the table at t = 0 as far as the host knows it -- common fields, HELD entries at their start; the first advance writes the rest -- and the clock
int reset_obstacles(const lscqp_plan_s::Obstacles& o) {
    std::vector<lscqp_obstacle> tab((size_t)o.n_dyn);
    memset(tab.data(), 0, tab.size() * sizeof(lscqp_obstacle));
    for (int i = 0; i < o.n_dyn; i++) {
        const lscqp_obstacle_model& m = o.models[(size_t)i];
        for (int k = 0; k < 3; k++) tab[(size_t)i].position[k] = (double)(float)m.start[k];
        tab[(size_t)i].radius = m.radius, tab[(size_t)i].downwash = m.downwash, tab[(size_t)i].max_acc = m.max_acc;
    }
    hipError_t e = hipMemcpy(o.table.get(), tab.data(), tab.size() * sizeof(lscqp_obstacle), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(o.clock.get(), 0, (size_t)o.n_tables * sizeof(int32_t));
    if (e == hipSuccess && o.drv.d_drives) e = hipMemset(o.drv.state.get(), 0, (size_t)o.n_dyn * sizeof(lscqp_obstacle_drive_state));
    return e == hipSuccess ? LSCQP_OK : hip_fail(e, "plan reset (obstacles)");
}

// the partition in force as offsets: [0, n_total] without one
std::vector<int64_t> mission_offsets_of(const lscqp_plan_s* p) {
    return p->mis.moff.empty() ? std::vector<int64_t>{0, p->s.n_total} : p->mis.moff;
}

// whose table is whose, as offsets over the local agents: the partition in force where table k belongs to mission k, else [0, n_agents]
std::vector<int64_t> table_owners_of(const lscqp_plan_s* p, bool per_mission) {
    return per_mission ? mission_offsets_of(p) : std::vector<int64_t>{0, p->s.n_agents};
}

// ids [n_agents][n_slot]: agent a of owners' block k names ooff[k] + j in slot j < count_k, -1 beyond
int upload_mission_ids(const lscqp_plan_s::Obstacles& o, const std::vector<int64_t>& owners, int64_t n_agents) {
    const size_t ns = (size_t)o.n_slot;
    std::vector<int32_t> hid((size_t)(n_agents ? n_agents : 1) * ns, -1);
    for (size_t k = 0; k + 1 < owners.size(); k++)
        for (int64_t a = owners[k]; a < owners[k + 1]; a++)
            for (int32_t j = 0; j < o.ooff[k + 1] - o.ooff[k]; j++) hid[(size_t)a * ns + (size_t)j] = o.ooff[k] + j;
    const hipError_t e = hipMemcpy(o.ids.get(), hid.data(), hid.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    return e == hipSuccess ? LSCQP_OK : hip_fail(e, o.per_mission ? "lscqp_plan_set_mission_obstacles (ids)" : "lscqp_plan_set_obstacles");
}

// a chaser of a table per mission follows an agent of the mission that owns it (target_agent >= 0), or a goal point
int check_chasers_stay_home(const lscqp_plan_s::Obstacles& o, const lscqp_obstacle_drive* drives, const std::vector<int64_t>& moff) {
    for (size_t k = 0; k + 1 < o.ooff.size() && k + 1 < moff.size(); k++)
        for (int32_t i = o.ooff[k]; i < o.ooff[k + 1]; i++) {
            const lscqp_obstacle_drive& d = drives[i];
            if (d.kind == LSCQP_DRIVE_CHASING && d.target_agent >= 0 && (d.target_agent < moff[k] || d.target_agent >= moff[k + 1]))
                return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, ("lscqp_plan_set_obstacle_drives: model " + std::to_string(i) + ": target_agent " +
                                                                     std::to_string(d.target_agent) + " lies outside mission " + std::to_string(k) +
                                                                     ", which owns the chaser (lscqp_plan_set_mission_obstacles)").c_str());
        }
    return LSCQP_OK;
}

// the plan's grid and the buffers sized by it (waypoint_mode 1): made at lscqp_plan_create, again by lscqp_plan_set_grid
int make_grid(lscqp_plan_s* p, double resolution) {
    lscqp_grid_desc gd;
    memset(&gd, 0, sizeof gd);
    gd.resolution = resolution, gd.radius = p->wp.radius, gd.z_2d = p->d.z_2d, gd.world_dimension = p->s.dim;
    decltype(p->wp.grid) gnew;
    {
        lscqp_grid g = nullptr;
        PLAN_TRY(lscqp_grid_create(p->map, &gd, &g));
        gnew.reset(g);
    }
    if (p->wld.set) PLAN_TRY(lscqp_grid_set_worlds(gnew.get(), p->wld.set));  // (a new grid of a plan with worlds gets them again)
    double gmin[3];
    int32_t dims[3];
    lscqp_grid_info(gnew.get(), gmin, dims);
    dev_ptr<int32_t> f, fo;
    PLAN_TRY(lscqp::dev_alloc(f, (size_t)p->s.n_total * dims[0] * dims[1], "hipMalloc(distance fields)"));
    if (p->pat.on) PLAN_TRY(lscqp::dev_alloc(fo, (size_t)p->s.n_total * dims[0] * dims[1], "hipMalloc(distance fields)"));  // (a patrol: both legs)
    PLAN_TRY(p->n_missions() > 1 ? lscqp_grid_reserve_missions_(gnew.get(), p->s.n_total, p->n_missions()) : lscqp_grid_reserve(gnew.get(), p->s.n_total));
    if (p->wp.decision != LSCQP_DECISION_ONE_WORKGROUP) PLAN_TRY(lscqp_grid_reserve_wide(gnew.get(), p->s.n_total));
    p->wp.grid = std::move(gnew);
    p->wp.field = std::move(f);
    p->wp.field_nodes = (size_t)dims[0] * dims[1];
    if (p->pat.on) p->pat.field_other = std::move(fo);
    p->wp.resolution = resolution;
    p->wp.fields_valid = false;
    return LSCQP_OK;
}

// updateGridMission + createDistanceTable for the whole mission (include/lscqp.h, DIFFERENCE 1); synchronous
int make_fields(lscqp_plan_s* p) {
    lscqp_plan_s::Waypoints& wp = p->wp;
    if (p->n_missions() > 1)
        PLAN_TRY(lscqp_grid_fields_missions_device(wp.grid.get(), p->s.n_total, p->n_missions(), p->mis.moff.data(), p->mis.d_moff.get(), wp.start_pts,
                                                   (const double*)p->buf[LSCQP_PLAN_BUF_DESIRED_GOAL], wp.field.get(), wp.init_d, nullptr));
    else
        PLAN_TRY(lscqp_grid_fields_device(wp.grid.get(), p->s.n_total, wp.start_pts, (const double*)p->buf[LSCQP_PLAN_BUF_DESIRED_GOAL], wp.field.get(), wp.init_d, nullptr));
    // a patrol: the opposite leg, by the same entry with starts and goals exchanged (the same nodes are cleared: one mission occupancy)
    if (p->pat.on && p->n_missions() > 1)
        PLAN_TRY(lscqp_grid_fields_missions_device(wp.grid.get(), p->s.n_total, p->n_missions(), p->mis.moff.data(), p->mis.d_moff.get(),
                                                   (const double*)p->buf[LSCQP_PLAN_BUF_DESIRED_GOAL], wp.start_pts, p->pat.field_other.get(), p->pat.init_d_other.get(), nullptr));
    else if (p->pat.on)
        PLAN_TRY(lscqp_grid_fields_device(wp.grid.get(), p->s.n_total, (const double*)p->buf[LSCQP_PLAN_BUF_DESIRED_GOAL], wp.start_pts, p->pat.field_other.get(),
                                          p->pat.init_d_other.get(), nullptr));
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "distance fields");
    wp.fields_valid = true;
    return LSCQP_OK;
}

// the flight log of a plan's record: `capacity` rows per mission with the obstacle columns and the table of `o` (capacity 0: none)
int give_log(lscqp_record r, int32_t capacity, const lscqp_plan_s::Obstacles& o) {
    PLAN_TRY(lscqp_record_set_log(r, capacity, o.n_dyn));
    if (capacity > 0) PLAN_TRY(lscqp_record_log_obstacles(r, o.n_dyn > 0 ? o.table.get() : nullptr));
    return LSCQP_OK;
}

// the plan's record for the partition in force (its offsets are the ones the partition already has on the device); the old one is dropped
int make_record(lscqp_plan_s* p, const lscqp_record_desc& desc) {
    lscqp_record rnew = nullptr;
    const bool one = p->mis.moff.empty();
    PLAN_TRY(lscqp_record_create_(p->h, p->s.n_total, one ? 1 : p->n_missions(), one ? nullptr : p->mis.moff.data(), one ? nullptr : p->mis.d_moff.get(),
                                  p->d.safety_samples, p->d.record_time_step, p->d.time_step, p->s.z_2d, &desc, &rnew));
    decltype(p->rec.held) made(rnew);
    PLAN_TRY(give_log(made.get(), p->rec.log_capacity, p->obs));
    if (p->rec.obstacle_figures) PLAN_TRY(lscqp_record_set_obstacle_figures(made.get(), p->obs.safety.get()));
    drop_graph(p);  // (a captured chain holds the old record's buffers)
    p->rec.held = std::move(made);
    return LSCQP_OK;
}

// The plan's obstacles, new: n_tables tables by their offsets (n_tables = 0: none), `prepared` their models, table k mission k's own
// (per_mission) or the one table everybody's.  `what` names the setter.  Everything that can fail comes before the plan changes
int set_obstacle_tables(lscqp_plan_s* p, const char* what, const lscqp_obstacle_param* param, int32_t n_tables, const int32_t* offsets,
                        std::vector<lscqp_obstacle_model>& prepared, bool per_mission) {
    OnDevice on(p->device);
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, what);
    const bool none = n_tables == 0;
    lscqp_plan_s::Obstacles next;  // (none: empty)
    if (!none) {
        const size_t n = (size_t)p->s.n_agents, T = (size_t)n_tables;
        next.ooff.assign(offsets, offsets + T + 1);
        next.n_tables = n_tables, next.n_dyn = offsets[T], next.per_mission = per_mission;
        for (size_t k = 0; k < T; k++) next.n_slot = std::max(next.n_slot, offsets[k + 1] - offsets[k]);
        const size_t nd = (size_t)next.n_dyn;
        PLAN_TRY(lscqp::dev_alloc(next.d_models, nd, what));
        PLAN_TRY(lscqp::dev_alloc(next.table, nd, what));
        PLAN_TRY(lscqp::dev_alloc(next.ids, (n ? n : 1) * (size_t)next.n_slot, what));
        PLAN_TRY(lscqp::dev_alloc(next.clock, T, what));
        PLAN_TRY(lscqp::dev_alloc(next.d_ooff, T + 1, what));
        PLAN_TRY(lscqp::dev_alloc(next.safety, n ? n : 1, what, true));
        e = hipMemcpy(next.d_models.get(), prepared.data(), nd * sizeof(lscqp_obstacle_model), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(next.d_ooff.get(), offsets, (T + 1) * sizeof(int32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_fail(e, what);
        PLAN_TRY(upload_mission_ids(next, table_owners_of(p, per_mission), p->s.n_agents));
        next.models.swap(prepared);
        next.param = *param;
        PLAN_TRY(reset_obstacles(next));  // (so that the table can be read, and HELD entries written, before the reset)
    }
    // (a flight log has the obstacles' columns and reads their table: a new log for the new ones, before the plan changes)
    if (p->rec.held && p->rec.log_capacity > 0) PLAN_TRY(give_log(p->rec.held.get(), p->rec.log_capacity, next));
    // (an obstacle record reads the obstacles' safety buffer: the new one, or none -- it goes with the obstacles)
    if (p->rec.held && p->rec.obstacle_figures) PLAN_TRY(lscqp_record_set_obstacle_figures(p->rec.held.get(), none ? nullptr : next.safety.get()));
    if (none) {
        p->rec.obstacle_figures = false;
        p->pending &= ~lscplan::kPendObstacleRecord;
    }
    drop_graph(p);  // (a captured chain holds the obstacles' nodes and the slot split)
    p->obs = std::move(next);
    // (the drives, and the other setter's obstacles, went with the old ones)
    p->pending &= ~(lscplan::kPendObstacles | lscplan::kPendMissionObstacles | lscplan::kPendDrives);
    if (!none) p->pending |= per_mission ? lscplan::kPendMissionObstacles : lscplan::kPendObstacles;
    return LSCQP_OK;
}

// The class constants travel to the kernels BY VALUE and the map view (table pointer + margin) likewise, so a captured graph -- and
// the private WARM_TIGHT clone of the handle -- are snapshots.  lscqp_update(h) (TrajOptimizer::updateParam, src/traj_optimizer.cpp:158-160)
// or lscqp_map_prepare after the capture would be silently ignored by the replayed graph while the eager chain sees the new values:
// compare the generation counters before every step, drop the graph and re-derive the clone when they moved.
int refresh(lscqp_plan_s* p) {
    const uint64_t hg = lscqp_handle_generation_(p->h), mg = p->map ? lscqp_map_generation_(p->map) : 0;
    const uint64_t wg = p->wld.set ? lscqp_worlds_generation_(p->wld.set) : 0;  // (every member map of a plan with worlds)
    if (hg == p->h_gen && mg == p->map_gen && wg == p->wld.gen) return LSCQP_OK;
    drop_graph(p);
    if (p->wld.set) PLAN_TRY(lscqp_worlds_refresh_(p->wld.set));  // (the set's table follows its members before anything is enqueued)
    if (hg != p->h_gen) {
        // the buffers and the launch shapes of prepare / commit were sized at lscqp_plan_create: an update that changes the SHAPE of the
        // class (segments, dimension, corridor rows on / off, row format, a kernel capacity below the plan's neighbour slots) cannot be
        // followed -- refuse the step instead of reading and writing x_new / x_init / rows out of bounds.  Such a plan has to be
        // destroyed and created again; every other field of the class (weights, dt-independent limits, modes) is followed.
        const lscqp_class_desc* now = lscqp_class_desc_of_(p->h);
        const int M = lscqp_num_segments(p->h), nv = lscqp_num_variables(p->h);
        if (M != p->s.M || nv != p->s.nv || (lscqp_uses_sfc(p->h) != 0) != (p->map != nullptr) || lscqp_max_obstacles(p->h) < p->s.n_obs ||
            lscqp_row_bytes(p->h) != (int)sizeof(lscqp_row) || !(p->d.time_step <= now->dt * (1 + 1e-9)))
            return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT,
                                    "lscqp_update changed the shape of the class (segments / dimension / corridor rows / row format / neighbour "
                                    "capacity / dt below the plan's time_step) under a live plan: destroy the plan and create it again");
        p->s.dt = now->dt;
        lscqp_class_desc cd = *now;
        if (p->d.tight_warm_start && cd.warm_start != LSCQP_WARM_TIGHT) {
            cd.warm_start = LSCQP_WARM_TIGHT;
            if (p->own_hq) {
                const int rc = lscqp_update(p->hq, &cd);
                if (rc != LSCQP_OK) return rc;
            } else {  // h was WARM_TIGHT itself when the plan was made and no longer is: the clone becomes necessary now
                lscqp_handle hq = nullptr;
                const int rc = lscqp_create(&cd, &hq);
                if (rc != LSCQP_OK) return rc;
                p->own_hq.reset(hq);
                p->hq = hq;
            }
        } else if (p->own_hq) {  // h became WARM_TIGHT itself: the clone only has to follow it
            const int rc = lscqp_update(p->hq, &cd);
            if (rc != LSCQP_OK) return rc;
        }
        if (p->own_hq && lscqp_prescreen(p->hq) != lscqp_prescreen(p->h)) {  // (lscqp_set_prescreen moves the generation too: the clone follows the mode)
            const int rc = lscqp_set_prescreen(p->hq, lscqp_prescreen(p->h));
            if (rc != LSCQP_OK) return rc;
        }
    }
    if ((mg != p->map_gen || wg != p->wld.gen) && p->wp.grid && p->wp.fields_valid) {  // the map moved under the mission: its grid and fields are made again
        const int rc = make_grid(p, p->wp.resolution);
        if (rc != LSCQP_OK) return rc;
        const int rc2 = make_fields(p);
        if (rc2 != LSCQP_OK) return rc2;
    }
    p->h_gen = hg;
    p->map_gen = mg;
    p->wld.gen = wg;
    return LSCQP_OK;
}

// the per-agent world index of a plan with worlds: the agent's mission in the partition `off` ([K + 1]); a fresh device array
int make_world_of(int64_t n_total, const int64_t* off, int K, dev_ptr<int32_t>& out) {
    std::vector<int32_t> host((size_t)n_total);
    for (int k = 0; k < K; k++)
        for (int64_t a = off[k]; a < off[k + 1]; a++) host[(size_t)a] = k;
    const char* const what = "world index of the agents";
    PLAN_TRY(lscqp::dev_alloc(out, host.size(), what));
    const hipError_t e = hipMemcpy(out.get(), host.data(), host.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        out.reset();
        return hip_fail(e, what);
    }
    return LSCQP_OK;
}

}  // namespace

extern "C" {

int lscqp_plan_create(lscqp_handle h, lscqp_map map, const lscqp_plan_desc* desc, const lscqp_agent_param* agents, lscqp_plan* out) {
    if (!h || !desc || !agents || !out) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null argument");
    // (n_agents == 0 is a legal plan: the empty last block of a mission sharded over more devices than ceil(N / G) blocks fill --
    // it holds the all-agent buffers, takes part in lscqp_plan_group_step's exchange and replans nothing)
    if (desc->n_agents < 0 || desc->n_total <= 0 || desc->first_agent < 0 || desc->n_total < desc->first_agent + desc->n_agents)
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "inconsistent sizes (n_agents >= 0, n_total > 0, n_total >= first_agent + n_agents required)");
    if (desc->n_obs < 0) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "negative n_obs");
    if (desc->n_obs > lscqp_max_obstacles(h))
        return lscqp_set_error_(LSCQP_ERR_UNSUPPORTED, "n_obs exceeds the largest compiled kernel instance of the shape (lscqp_max_obstacles)");
    if (desc->constraint_mode != LSCQP_GEN_LSC && desc->constraint_mode != LSCQP_GEN_CLSC && desc->constraint_mode != LSCQP_GEN_BVC)
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "constraint_mode must be LSCQP_GEN_LSC, LSCQP_GEN_CLSC or LSCQP_GEN_BVC");
    if (desc->sfc_mode != LSCQP_SFC_FROM_HULL && desc->sfc_mode != LSCQP_SFC_FROM_POINT)
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "sfc_mode must be LSCQP_SFC_FROM_HULL or LSCQP_SFC_FROM_POINT");
    for (const int32_t mode : {desc->prediction_mode, desc->initial_traj_mode})
        if (mode != LSCQP_TRAJ_FROM_PREVIOUS_SOLUTION && mode != LSCQP_TRAJ_FROM_POSITION && mode != LSCQP_TRAJ_FROM_VELOCITY)
            return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "prediction_mode / initial_traj_mode must be LSCQP_TRAJ_FROM_PREVIOUS_SOLUTION, _FROM_POSITION or _FROM_VELOCITY");
    if (!(desc->reset_threshold == desc->reset_threshold)) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "reset_threshold is NaN");
    const int uses_sfc = lscqp_uses_sfc(h);
    if ((uses_sfc != 0) != (map != nullptr))
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "a map is required exactly when the solver class uses corridors (use_sfc)");
    const int M = lscqp_num_segments(h), nv = lscqp_num_variables(h);
    const double dt_probe = lscqp_class_desc_of_(h)->dt;
    if (!(desc->time_step > 0) || desc->time_step > dt_probe * (1 + 1e-9))
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "0 < time_step <= dt required (multisim_time_step, src/traj_planner.cpp:401-421)");
    if (desc->safety_samples < 0 || (desc->safety_samples > 0 && (desc->n_agents != desc->n_total || !(desc->record_time_step > 0))))
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT,
                                "safety_samples needs every agent's new plan on this device (n_agents == n_total) and record_time_step > 0");
    if (lscqp_row_bytes(h) != (int)sizeof(lscqp_row))
        return lscqp_set_error_(LSCQP_ERR_UNSUPPORTED, "the plan chain uses 32-byte rows (row_format = LSCQP_ROWS_F64)");
    if (desc->waypoint_mode != LSCQP_WAYPOINT_FROM_CALLER && desc->waypoint_mode != LSCQP_WAYPOINT_GRID_PIBT)
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "waypoint_mode must be LSCQP_WAYPOINT_FROM_CALLER or LSCQP_WAYPOINT_GRID_PIBT");
    if (desc->waypoint_mode == LSCQP_WAYPOINT_GRID_PIBT) {
        if (desc->n_agents != desc->n_total)
            return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "waypoint_mode = LSCQP_WAYPOINT_GRID_PIBT needs every agent's waypoint and plan on this device (n_agents == n_total)");
        if (!map) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "waypoint_mode = LSCQP_WAYPOINT_GRID_PIBT needs a map");
        if (nv / (6 * M) != 2) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "waypoint_mode = LSCQP_WAYPOINT_GRID_PIBT needs a 2-D class (the reference's MAPF graph is x-y only)");
    }
    if (map) {  // the corridor kernel's free-space table for the agents of this mission (no-op if the map already has one that serves them)
        double rmax = 0;
        for (int64_t i = 0; i < desc->n_total; i++) rmax = agents[i].radius > rmax ? agents[i].radius : rmax;
        if (rmax > 0) {
            const int rc = lscqp_map_prepare(map, rmax);
            if (rc != LSCQP_OK && rc != LSCQP_ERR_UNSUPPORTED) return rc;  // (a map too large for the table: the corridors work without it)
        }
    }
    int cur_dev = 0;
    if (hipGetDevice(&cur_dev) != hipSuccess) return lscqp_set_error_(LSCQP_ERR_NO_DEVICE, "no HIP device: lscqp has no CPU fallback");
    if (map && lscqp_map_device_(map) != cur_dev)
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT,
                                "the map lives on another device than the plan (create the map with the plan's device current: the corridor "
                                "kernel dereferences the map's grids)");
    std::unique_ptr<lscqp_plan_s, void (*)(lscqp_plan)> owner(new lscqp_plan_s(), lscqp_plan_destroy);
    lscqp_plan_s* p = owner.get();
    p->h = h;
    p->hq = h;
    p->device = cur_dev;
    if (desc->tight_warm_start && lscqp_class_desc_of_(h)->warm_start != LSCQP_WARM_TIGHT) {
        lscqp_class_desc cd = *lscqp_class_desc_of_(h);
        cd.warm_start = LSCQP_WARM_TIGHT;
        PLAN_TRY(lscqp_create(&cd, &p->hq));  // (lscqp_create has set the message)
        p->own_hq.reset(p->hq);
        if (lscqp_prescreen(h) != LSCQP_PRESCREEN_OFF) (void)lscqp_set_prescreen(p->hq, lscqp_prescreen(h));
    }
    p->h_gen = lscqp_handle_generation_(h);
    p->map_gen = map ? lscqp_map_generation_(map) : 0;
    p->map = map;
    p->d = *desc;
    p->s.M = M;
    p->s.dim = nv / (6 * M);
    p->s.nv = nv;
    p->s.n_obs = desc->n_obs;
    p->s.n_agents = desc->n_agents;
    p->s.n_total = desc->n_total;
    p->s.first_agent = desc->first_agent;
    p->s.z_2d = desc->z_2d;
    p->s.dt = dt_probe;
    p->s.prediction_mode = desc->prediction_mode;
    p->s.initial_traj_mode = desc->initial_traj_mode;
    p->s.reset_threshold = desc->reset_threshold;
    const size_t n = (size_t)desc->n_agents, nt = (size_t)desc->n_total, P = (size_t)M * 6, no = (size_t)desc->n_obs;
    int rc = LSCQP_OK;
    auto ok = [&](int r) { return rc == LSCQP_OK && (rc = r) == LSCQP_OK; };
    // (the three buffers a group exchanges carry room for LSCQP_PLAN_EXCHANGE_PAD agents behind the mission: a ragged split is then one
    // in-place all-gather of full blocks as well, include/lscqp.h; the public size stays the mission's)
    const size_t ntp = nt + LSCQP_PLAN_EXCHANGE_PAD;
    ok(dalloc_pub<double>(p, LSCQP_PLAN_BUF_STATE, ntp * 9)) && ok(dalloc_pub<double>(p, LSCQP_PLAN_BUF_WAYPOINT, n * 3)) &&
        ok(dalloc_pub<double>(p, LSCQP_PLAN_BUF_PLAN, ntp * nv)) && ok(dalloc_pub<double>(p, LSCQP_PLAN_BUF_GOAL, ntp * 3)) &&
        ok(dalloc_pub<lscqp_header>(p, LSCQP_PLAN_BUF_HEADER, n)) && ok(dalloc_pub<lscqp_row>(p, LSCQP_PLAN_BUF_ROWS, n * no * P)) &&
        ok(dalloc_pub<lscqp_box>(p, LSCQP_PLAN_BUF_SFC, n * M)) && ok(dalloc_pub<int32_t>(p, LSCQP_PLAN_BUF_STATUS, n)) &&
        ok(dalloc_pub<int32_t>(p, LSCQP_PLAN_BUF_GOAL_STATUS, n)) && ok(dalloc_pub<int32_t>(p, LSCQP_PLAN_BUF_SFC_STATUS, n)) &&
        ok(dalloc_pub<int32_t>(p, LSCQP_PLAN_BUF_VALID, n)) && ok(dalloc_pub<int32_t>(p, LSCQP_PLAN_BUF_IN_RANGE, n)) &&
        (desc->closed_loop ? true : ok(dalloc_pub<double>(p, LSCQP_PLAN_BUF_NEXT_STATE, n * 9))) && ok(dalloc_pub<double>(p, LSCQP_PLAN_BUF_OBJECTIVE, n)) &&
        ok(dalloc_pub<lscqp_info>(p, LSCQP_PLAN_BUF_INFO, n)) && ok(dalloc_pub<lscqp_safety>(p, LSCQP_PLAN_BUF_SAFETY, n)) && ok(dalloc(p, &p->par, nt)) && ok(dalloc(p, &p->radius, nt)) &&
        ok(dalloc(p, &p->downwash, nt)) && ok(dalloc(p, &p->traj, nt * P * 3)) && ok(dalloc(p, &p->pos, nt * 3)) &&
        ok(dalloc(p, &p->points, n * 9)) && ok(dalloc(p, &p->own, n * P * 3)) && ok(dalloc(p, &p->x_init, n * nv)) && ok(dalloc(p, &p->x_new, n * nv)) &&
        ok(dalloc(p, &p->nbr, n * no)) && ok(dalloc(p, &p->off, n + 1)) && ((int64_t)n > lscqp_launch_capacity(h, (int64_t)n, desc->n_obs) ? ok(dalloc(p, &p->order, n)) : true) &&
        ((map && n > lscplan::kSfcOrderMin) ? (ok(dalloc(p, &p->sfc_order, n)) && ok(dalloc(p, &p->sfc_cost, n))) : true);
    if (desc->waypoint_mode == LSCQP_WAYPOINT_GRID_PIBT) {
        ok(dalloc_pub<double>(p, LSCQP_PLAN_BUF_DESIRED_GOAL, nt * 3)) && ok(dalloc_pub<int32_t>(p, LSCQP_PLAN_BUF_WAYPOINT_UPDATED, n)) &&
            ok(dalloc_pub<int32_t>(p, LSCQP_PLAN_BUF_GROUP, n)) && ok(dalloc(p, &p->wp.init_d, nt)) && ok(dalloc(p, &p->wp.desired_node, nt)) && ok(dalloc(p, &p->wp.start_pts, nt * 3));
        p->wp.radius = agents[0].radius;  // (planMAPF is handed mission.agents[0].radius, src/multi_sync_simulator.cpp:211-214)
        if (rc == LSCQP_OK) rc = make_grid(p, 0.5);
    }
    if (rc == LSCQP_OK) {
        p->bytes[LSCQP_PLAN_BUF_STATE] = nt * 9 * sizeof(double);
        p->bytes[LSCQP_PLAN_BUF_PLAN] = nt * nv * sizeof(double);
        p->bytes[LSCQP_PLAN_BUF_GOAL] = nt * 3 * sizeof(double);
    }
    if (rc == LSCQP_OK && desc->closed_loop) {
        p->buf[LSCQP_PLAN_BUF_NEXT_STATE] = (double*)p->buf[LSCQP_PLAN_BUF_STATE] + desc->first_agent * 9;
        p->bytes[LSCQP_PLAN_BUF_NEXT_STATE] = n * 9 * sizeof(double);
    }
    if (rc == LSCQP_OK) {
        std::vector<double> r(nt), w(nt);
        std::vector<uint64_t> off(n + 1);
        for (size_t i = 0; i < nt; i++) {
            r[i] = agents[i].radius;
            w[i] = agents[i].downwash;
        }
        for (size_t i = 0; i <= n; i++) off[i] = (uint64_t)(i * no * P);
        hipError_t e = hipMemcpy(p->par, agents, nt * sizeof(lscqp_agent_param), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(p->radius, r.data(), nt * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(p->downwash, w.data(), nt * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(p->off, off.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&p->cap, hipStreamNonBlocking);
        if (e != hipSuccess) rc = hip_fail(e, "plan set-up");
    }
    if (rc != LSCQP_OK) return rc;
    *out = owner.release();
    return LSCQP_OK;
}

void lscqp_plan_destroy(lscqp_plan p) {
    if (!p) return;
    OnDevice on(p->device);
    (void)hipDeviceSynchronize();
    drop_graph(p);
    if (p->cap) (void)hipStreamDestroy(p->cap);
    delete p;
}

int lscqp_plan_reset(lscqp_plan p, const double* start_positions, const double* goal_points) {
    if (!p || !start_positions) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null argument");
    if (p->wp.grid && !goal_points) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "waypoint_mode = LSCQP_WAYPOINT_GRID_PIBT: the mission's goal points are required");
    if (p->rec.on && !goal_points) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_plan_set_record: the mission's goal points are required (the desired goals of the finish test)");
    if (p->pat.on && !goal_points) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_plan_set_patrol: the mission's goal points are required (the far end of every leg)");
    if (p->obs.per_mission) {  // a table per mission: of the partition in force, and every chaser after an agent of its own mission
        if (p->obs.n_tables != p->n_missions())
            return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, ("lscqp_plan_set_mission_obstacles: " + std::to_string(p->obs.n_tables) + " obstacle tables for " +
                                                                 std::to_string(p->n_missions()) + " missions: one table per mission of the partition in force required").c_str());
        if (!p->obs.drv.host.empty()) PLAN_TRY(check_chasers_stay_home(p->obs, p->obs.drv.host.data(), mission_offsets_of(p)));
    }
    OnDevice on(p->device);
    const lscplan::Shape& s = p->s;
    const size_t nt = (size_t)s.n_total, P = (size_t)s.M * 6;
    std::vector<double> st(nt * 9, 0.0), x(nt * s.nv), gl(nt * 3), dg(p->wp.grid ? nt * 3 : 0);
    for (size_t a = 0; a < nt; a++) {
        for (int k = 0; k < 3; k++) {
            // State holds point3d; a 2-D mission flies at z = world_z_2d (src/agent_manager.cpp:40-42)
            const double v = (k < s.dim) ? (double)(float)start_positions[a * 3 + k] : (double)(float)s.z_2d;
            st[a * 9 + k] = v;
            gl[a * 3 + k] = (goal_points && !p->wp.grid) ? (double)(float)goal_points[a * 3 + k] : v;  // AgentManager ctor: current_goal_point = start
            if (p->wp.grid) dg[a * 3 + k] = (k < s.dim) ? (double)(float)goal_points[a * 3 + k] : v;  // Agent::desired_goal_point, in the mission's plane
        }
        for (int k = 0; k < s.dim; k++)
            for (size_t j = 0; j < P; j++) x[a * s.nv + k * P + j] = st[a * 9 + k];
    }
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(p->buf[LSCQP_PLAN_BUF_STATE], st.data(), st.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->buf[LSCQP_PLAN_BUF_PLAN], x.data(), x.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->buf[LSCQP_PLAN_BUF_GOAL], gl.data(), gl.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->buf[LSCQP_PLAN_BUF_WAYPOINT], gl.data() + s.first_agent * 3, (size_t)s.n_agents * 3 * sizeof(double), hipMemcpyHostToDevice);
    if (p->wp.grid) {  // (gl holds the start positions here: the waypoints above start there, src/agent_manager.cpp:10)
        if (e == hipSuccess) e = hipMemcpy(p->buf[LSCQP_PLAN_BUF_DESIRED_GOAL], dg.data(), dg.size() * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(p->wp.start_pts, gl.data(), gl.size() * sizeof(double), hipMemcpyHostToDevice);
    }
    if (p->pat.on) {  // every agent on leg 0: the patrol's own buffers (the plan's were written above), no leg flown, nobody turned
        std::vector<double> sp(nt * 3), want(nt * 3);
        for (size_t a = 0; a < nt; a++)
            for (int k = 0; k < 3; k++) {
                sp[a * 3 + k] = st[a * 9 + k];
                want[a * 3 + k] = (k < s.dim) ? (double)(float)goal_points[a * 3 + k] : st[a * 9 + k];
            }
        if (e == hipSuccess && p->pat.own_start) e = hipMemcpy(p->pat.own_start.get(), sp.data(), sp.size() * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess && p->pat.own_desired) e = hipMemcpy(p->pat.own_desired.get(), want.data(), want.size() * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemset(p->pat.legs.get(), 0, nt * sizeof(int32_t));
        if (e == hipSuccess) e = hipMemset(p->pat.swapped.get(), 0, nt * sizeof(int32_t));
    }
    if (e != hipSuccess) return hip_fail(e, "plan reset");
    if (p->wp.grid) PLAN_TRY(make_fields(p));
    if (p->rec.on) {  // the record of the partition in force, cleared; desired goals in the mission's plane like the states
        if (!p->rec.held || (p->pending & (lscplan::kPendRecord | lscplan::kPendMissions))) PLAN_TRY(make_record(p, p->rec.desc));
        std::vector<double> want(nt * 3);
        for (size_t a = 0; a < nt; a++)
            for (int k = 0; k < 3; k++) want[a * 3 + k] = (k < s.dim) ? goal_points[a * 3 + k] : st[a * 9 + k];
        // a patrol never finishes (isFinished, src/multi_sync_simulator.cpp:401-404): desired goals at +infinity make every distance of the
        // record's finish test +inf, which exceeds any threshold -- the record's kernel is the one it always was
        if (p->pat.on) std::fill(want.begin(), want.end(), (double)INFINITY);
        PLAN_TRY(lscqp_record_reset(p->rec.held.get(), want.data()));
    }
    if (p->obs.n_dyn > 0) {  // the partition may have other offsets by now (never another count): each agent's own entries again
        PLAN_TRY(upload_mission_ids(p->obs, table_owners_of(p, p->obs.per_mission), s.n_agents));
        PLAN_TRY(reset_obstacles(p->obs));
    }
    p->pending = 0;
    p->first = true;
    p->steps = 0;
    return LSCQP_OK;
}

void* lscqp_plan_buffer(lscqp_plan p, int32_t which, uint64_t* bytes_out) {
    if (!p || which < 0 || which >= LSCQP_PLAN_BUF_COUNT) {
        lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "unknown plan buffer");
        return nullptr;
    }
    if (bytes_out) *bytes_out = p->bytes[which];
    return p->buf[which];
}

int lscqp_plan_upload(lscqp_plan p, int32_t which, const void* host, uint64_t offset, uint64_t bytes) {
    if (!p || !host || which < 0 || which >= LSCQP_PLAN_BUF_COUNT) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "bad argument");
    if (offset + bytes > p->bytes[which]) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "range exceeds the buffer");
    OnDevice on(p->device);
    const hipError_t e = hipMemcpy((char*)p->buf[which] + offset, host, bytes, hipMemcpyHostToDevice);
    return e == hipSuccess ? LSCQP_OK : hip_fail(e, "plan upload");
}

int lscqp_plan_download(lscqp_plan p, int32_t which, void* host, uint64_t offset, uint64_t bytes) {
    if (!p || !host || which < 0 || which >= LSCQP_PLAN_BUF_COUNT) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "bad argument");
    if (offset + bytes > p->bytes[which]) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "range exceeds the buffer");
    OnDevice on(p->device);
    const hipError_t e = hipMemcpy(host, (const char*)p->buf[which] + offset, bytes, hipMemcpyDeviceToHost);  // waits for the device
    return e == hipSuccess ? LSCQP_OK : hip_fail(e, "plan download");
}

int lscqp_plan_step(lscqp_plan p, void* stream) {
    if (!p) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null plan");
    OnDevice on(p->device);
    PLAN_TRY(refresh(p));
    PLAN_TRY(may_step(p));
    PLAN_TRY(enqueue(p, p->first, (hipStream_t)stream));
    p->first = false;
    p->steps++;
    return LSCQP_OK;
}

int lscqp_plan_step_graph(lscqp_plan p, void* stream) {
    if (!p) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null plan");
    // the first replan differs (initializeSFC) and it also warms the kernels' one-time function attributes up: eager
    if (p->first || p->s.n_agents == 0) return lscqp_plan_step(p, stream);
    OnDevice on(p->device);
    PLAN_TRY(refresh(p));
    PLAN_TRY(may_step(p));
    if (!p->exec) {
        hipError_t e = hipStreamBeginCapture(p->cap, hipStreamCaptureModeThreadLocal);
        if (e != hipSuccess) return hip_fail(e, "hipStreamBeginCapture");
        const int rc = enqueue(p, false, p->cap);
        hipGraph_t gr = nullptr;
        e = hipStreamEndCapture(p->cap, &gr);
        if (rc != LSCQP_OK) {
            if (gr) (void)hipGraphDestroy(gr);
            return rc;
        }
        if (e != hipSuccess) return hip_fail(e, "hipStreamEndCapture");
        p->graph = gr;
        e = hipGraphInstantiate(&p->exec, gr, nullptr, nullptr, 0);
        if (e != hipSuccess) {
            drop_graph(p);
            return hip_fail(e, "hipGraphInstantiate");
        }
    }
    const hipError_t e = hipGraphLaunch(p->exec, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "hipGraphLaunch");
    p->steps++;
    return LSCQP_OK;
}

int lscqp_plan_set_grid(lscqp_plan p, double resolution) {
    if (!p) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null plan");
    if (!p->wp.grid) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "the plan has no grid (waypoint_mode = LSCQP_WAYPOINT_FROM_CALLER)");
    OnDevice on(p->device);
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "lscqp_plan_set_grid");
    drop_graph(p);  // (a captured chain holds the old grid's buffers)
    return make_grid(p, resolution);
}

lscqp_grid lscqp_plan_grid(lscqp_plan p) { return p ? p->wp.grid.get() : nullptr; }

int lscqp_plan_set_missions(lscqp_plan p, int32_t n_missions, const int64_t* mission_offsets) {
    if (!p) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null plan");
    const bool single = n_missions <= 1 || !mission_offsets;
    if (p->wld.set && (single ? 1 : n_missions) != lscqp_worlds_count_(p->wld.set))
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT,
                                ("lscqp_plan_set_missions: the plan has " + std::to_string(lscqp_worlds_count_(p->wld.set)) +
                                 " worlds (lscqp_plan_set_worlds), one per mission: another mission count needs other worlds, or none, first").c_str());
    if (p->obs.per_mission && (single ? 1 : n_missions) != p->obs.n_tables)
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT,
                                ("lscqp_plan_set_missions: the plan has " + std::to_string(p->obs.n_tables) +
                                 " obstacle tables (lscqp_plan_set_mission_obstacles), one per mission: another mission count needs other obstacles, or none, first").c_str());
    if (!single) {
        if (p->s.n_agents != p->s.n_total)
            return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "a mission partition needs every agent on this device (n_agents == n_total): a sharded plan flies one mission");
        PLAN_TRY(lscqp_check_missions_(p->s.n_total, n_missions, mission_offsets));
        if (p->wp.decision != LSCQP_DECISION_ONE_WORKGROUP)
            return lscqp_set_error_(LSCQP_ERR_UNSUPPORTED, "a partition of more than one mission keeps one workgroup per mission: set LSCQP_DECISION_ONE_WORKGROUP first");
    }
    OnDevice on(p->device);
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "lscqp_plan_set_missions");
    lscqp_plan_s::Missions next;  // (one mission: empty)
    dev_ptr<int32_t> wof;
    if (!single) {
        next.moff.assign(mission_offsets, mission_offsets + n_missions + 1);
        PLAN_TRY(lscqp::dev_alloc(next.d_moff, next.moff.size(), "lscqp_plan_set_missions"));
        e = hipMemcpy(next.d_moff.get(), mission_offsets, next.moff.size() * sizeof(int64_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_fail(e, "lscqp_plan_set_missions");
        if (p->wp.grid) PLAN_TRY(lscqp_grid_reserve_missions_(p->wp.grid.get(), p->s.n_total, n_missions));
        // worlds are set (the count is theirs): the agents' world index follows the NEW offsets -- an agent that changes mission changes world
        if (p->wld.set) PLAN_TRY(make_world_of(p->s.n_total, mission_offsets, n_missions, wof));
    }
    if (wof) p->wld.world_of = std::move(wof);
    p->mis = std::move(next);
    drop_graph(p);  // (a captured chain holds the old partition's launches)
    p->wp.fields_valid = false;
    p->rec.held.reset();  // (the record was built for the old partition and reads its device offsets: made again at the reset)
    p->pending |= lscplan::kPendMissions | (p->rec.on ? lscplan::kPendRecord : 0u);
    return LSCQP_OK;
}

int lscqp_plan_set_worlds(lscqp_plan p, lscqp_worlds worlds) {
    if (!p) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null plan");
    const lscplan::Shape& s = p->s;
    if (worlds) {
        const int K = lscqp_worlds_count_(worlds);
        if (p->mis.moff.empty())
            return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_plan_set_worlds: the plan has no mission partition (lscqp_plan_set_missions first): world k belongs to mission k");
        if (K != p->n_missions())
            return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, ("lscqp_plan_set_worlds: " + std::to_string(K) + " worlds for " + std::to_string(p->n_missions()) +
                                                                 " missions: one world per mission required").c_str());
        if (!p->map)
            return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_plan_set_worlds: the plan's class has no corridors (use_sfc = 0) and its grid no map: nothing in its chain reads a world");
        if (const char* f = lscqp_worlds_shape_difference_(worlds, p->map))
            return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT,
                                    (std::string("lscqp_plan_set_worlds: the worlds differ from the map the plan was created with in ") + f).c_str());
    }
    OnDevice on(p->device);
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "lscqp_plan_set_worlds");
    lscqp_plan_s::Worlds next;
    lscqp_grid grid = p->wp.grid.get();
    if (worlds) {  // (everything that can fail comes before the plan changes)
        const size_t nt = (size_t)s.n_total;
        std::vector<double> r(nt);
        e = hipMemcpy(r.data(), p->radius, nt * sizeof(double), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hip_fail(e, "lscqp_plan_set_worlds");
        double rmax = 0;
        for (const double v : r) rmax = v > rmax ? v : rmax;
        PLAN_TRY(make_world_of(s.n_total, p->mis.moff.data(), p->n_missions(), next.world_of));
        int rc = grid ? lscqp_grid_set_worlds(grid, worlds) : LSCQP_OK;
        // The free-space tables for the agents of this plan, one margin for all worlds -- LAST of what can fail, because it is the one step
        // that reaches beyond the plan: it may rebuild the members' tables, which moves their generation counters (include/lscqp.h).  A
        // failure behind the grid's change puts the grid back
        if (rc == LSCQP_OK && rmax > 0) {
            rc = lscqp_worlds_prepare(worlds, rmax);
            if (rc == LSCQP_ERR_UNSUPPORTED) rc = LSCQP_OK;  // (maps too large for the table: the corridors work without it)
            if (rc != LSCQP_OK && grid) (void)lscqp_grid_set_worlds(grid, p->wld.set);
        }
        if (rc != LSCQP_OK) return rc;
        next.set = worlds;
        next.gen = lscqp_worlds_generation_(worlds);
    } else if (grid) {
        PLAN_TRY(lscqp_grid_set_worlds(grid, nullptr));
    }
    drop_graph(p);  // (a captured chain holds the other corridor node)
    p->wld = std::move(next);
    if (p->map) p->map_gen = lscqp_map_generation_(p->map);  // (the plan's own map may be a member just prepared: nothing derived from it is left)
    p->wp.fields_valid = false;
    p->pending |= lscplan::kPendWorlds;
    return LSCQP_OK;
}

int lscqp_plan_set_waypoint_decision(lscqp_plan p, int32_t which) {
    if (!p) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null plan");
    if (which != LSCQP_DECISION_ONE_WORKGROUP && which != LSCQP_DECISION_WIDE && which != LSCQP_DECISION_AUTO)
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "which must be LSCQP_DECISION_ONE_WORKGROUP, LSCQP_DECISION_WIDE or LSCQP_DECISION_AUTO");
    if (!p->wp.grid) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "the plan decides no waypoints (waypoint_mode = LSCQP_WAYPOINT_FROM_CALLER)");
    if (which != LSCQP_DECISION_ONE_WORKGROUP && p->n_missions() > 1)
        return lscqp_set_error_(LSCQP_ERR_UNSUPPORTED, "a partition of more than one mission keeps one workgroup per mission");
    OnDevice on(p->device);
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "lscqp_plan_set_waypoint_decision");
    if (which != LSCQP_DECISION_ONE_WORKGROUP) PLAN_TRY(lscqp_grid_reserve_wide(p->wp.grid.get(), p->s.n_total));  // (before the plan changes)
    drop_graph(p);  // (a captured chain holds the other form's launches)
    p->wp.decision = which;
    return LSCQP_OK;
}

int lscqp_plan_missions(lscqp_plan p, int32_t* n_missions_out, int64_t* offsets_out) {
    if (!p || !n_missions_out) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null argument");
    const int K = p->n_missions();
    *n_missions_out = K;
    if (offsets_out) {
        if (K > 1) memcpy(offsets_out, p->mis.moff.data(), (size_t)(K + 1) * sizeof(int64_t));
        else offsets_out[0] = 0, offsets_out[1] = p->s.n_total;
    }
    return LSCQP_OK;
}

int lscqp_plan_mission_status(lscqp_plan p, int32_t* status_out) {
    if (!p || !status_out) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null argument");
    const int K = p->n_missions();
    if (!p->wp.grid) {  // (no waypoint walk in this plan: nothing to report)
        for (int k = 0; k < K; k++) status_out[k] = 0;
        return LSCQP_OK;
    }
    OnDevice on(p->device);
    return K > 1 ? lscqp_grid_mission_status(p->wp.grid.get(), K, status_out) : lscqp_grid_status(p->wp.grid.get(), status_out);
}

int lscqp_plan_set_record(lscqp_plan p, const lscqp_record_desc* desc) {
    if (!p) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null plan");
    if (desc) {
        if (p->d.safety_samples <= 0)
            return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_plan_set_record: the record reads the safety figures of the chain (safety_samples > 0 required)");
        if (p->s.n_agents != p->s.n_total)
            return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_plan_set_record: the record needs every agent on this device (n_agents == n_total)");
        if (!(desc->goal_threshold >= 0)) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_plan_set_record: goal_threshold must be >= 0");
    }
    OnDevice on(p->device);
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "lscqp_plan_set_record");
    if (!desc) {
        drop_graph(p);  // (a captured chain ends in the record's node)
        p->rec = {};  // (its flight log and its obstacle record with it)
        p->pending &= ~(lscplan::kPendRecord | lscplan::kPendFlightLog | lscplan::kPendObstacleRecord);
        return LSCQP_OK;
    }
    // (with the partition pending its device offsets are about to change: lscqp_plan_reset makes the record)
    if (!(p->pending & lscplan::kPendMissions)) PLAN_TRY(make_record(p, *desc));
    drop_graph(p);
    p->rec.desc = *desc;
    p->rec.on = true;
    p->pending |= lscplan::kPendRecord;
    return LSCQP_OK;
}

lscqp_record lscqp_plan_record(lscqp_plan p) { return p ? p->rec.held.get() : nullptr; }

int lscqp_plan_set_flight_log(lscqp_plan p, int32_t max_replans) {
    if (!p) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null plan");
    if (max_replans < 0) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_plan_set_flight_log: max_replans >= 0 required");
    if (!p->rec.on)
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_plan_set_flight_log: the plan has no record (lscqp_plan_set_record first): the log is part of it");
    if (max_replans > 0 && p->obs.per_mission)
        return lscqp_set_error_(LSCQP_ERR_UNSUPPORTED, "lscqp_plan_set_flight_log: the plan has a table of obstacles per mission (lscqp_plan_set_mission_obstacles); the log's obstacle columns are those of one shared table");
    OnDevice on(p->device);
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "lscqp_plan_set_flight_log");
    // (without a record in hand -- the partition is pending -- lscqp_plan_reset makes one, with the log)
    if (p->rec.held) PLAN_TRY(give_log(p->rec.held.get(), max_replans, p->obs));
    drop_graph(p);  // (a captured chain has, or lacks, the log's node)
    p->rec.log_capacity = max_replans;
    p->pending = max_replans > 0 ? p->pending | lscplan::kPendFlightLog : p->pending & ~lscplan::kPendFlightLog;
    return LSCQP_OK;
}

int lscqp_plan_set_obstacle_record(lscqp_plan p, int32_t on) {
    if (!p) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null plan");
    if (on && !p->rec.on)
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_plan_set_obstacle_record: the plan has no record (lscqp_plan_set_record first): the obstacle record is part of it");
    if (on && p->obs.n_dyn == 0)
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_plan_set_obstacle_record: the plan has no obstacles (lscqp_plan_set_obstacles first)");
    OnDevice dev(p->device);
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "lscqp_plan_set_obstacle_record");
    // (without a record in hand -- the partition is pending -- lscqp_plan_reset makes one, with the figures)
    if (p->rec.held) PLAN_TRY(lscqp_record_set_obstacle_figures(p->rec.held.get(), on ? p->obs.safety.get() : nullptr));
    drop_graph(p);  // (a captured chain has, or lacks, the obstacle record's node)
    p->rec.obstacle_figures = on != 0;
    p->pending = on ? p->pending | lscplan::kPendObstacleRecord : p->pending & ~lscplan::kPendObstacleRecord;
    return LSCQP_OK;
}

int lscqp_plan_set_obstacles(lscqp_plan p, const lscqp_obstacle_param* param, int32_t n_dyn, const lscqp_obstacle_model* models) {
    if (!p) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null plan");
    if (n_dyn < 0) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_plan_set_obstacles: negative n_dyn");
    const bool none = n_dyn == 0 || !models;
    std::vector<lscqp_obstacle_model> prepared;
    if (!none) {
        if (!param) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_plan_set_obstacles: null param");
        if (n_dyn > p->s.n_obs)
            return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_plan_set_obstacles: n_dyn exceeds the plan's row slots per agent (n_dyn <= desc.n_obs required)");
        if (p->d.constraint_mode != LSCQP_GEN_LSC && p->d.constraint_mode != LSCQP_GEN_CLSC)
            return lscqp_set_error_(LSCQP_ERR_UNSUPPORTED, "lscqp_plan_set_obstacles: constraint_mode must be LSCQP_GEN_LSC or LSCQP_GEN_CLSC (generateBVC's obstacle rows are not built)");
        prepared.assign(models, models + n_dyn);
        PLAN_TRY(lscqp_obstacle_model_prepare(prepared.data(), n_dyn));
    }
    const int32_t offsets[2] = {0, n_dyn};  // (one table, everybody's)
    return set_obstacle_tables(p, "lscqp_plan_set_obstacles", param, none ? 0 : 1, offsets, prepared, false);
}

int lscqp_plan_set_mission_obstacles(lscqp_plan p, const lscqp_obstacle_param* param, int32_t n_missions, const int32_t* obstacle_offsets,
                                     const lscqp_obstacle_model* models) {
    const char* const what = "lscqp_plan_set_mission_obstacles";
    if (!p) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null plan");
    if (n_missions < 0) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_plan_set_mission_obstacles: negative n_missions");
    // (no mission, no models, or missions none of which owns an obstacle: the obstacles are taken away, as lscqp_plan_set_obstacles does it)
    bool none = n_missions == 0 || !models;
    if (!none && obstacle_offsets) none = std::all_of(obstacle_offsets, obstacle_offsets + n_missions + 1, [](int32_t v) { return v == 0; });
    if (none) return lscqp_plan_set_obstacles(p, nullptr, 0, nullptr);
    if (!param) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_plan_set_mission_obstacles: null param");
    if (!obstacle_offsets) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_plan_set_mission_obstacles: null obstacle_offsets");
    if (p->d.constraint_mode != LSCQP_GEN_LSC && p->d.constraint_mode != LSCQP_GEN_CLSC)
        return lscqp_set_error_(LSCQP_ERR_UNSUPPORTED, "lscqp_plan_set_mission_obstacles: constraint_mode must be LSCQP_GEN_LSC or LSCQP_GEN_CLSC (generateBVC's obstacle rows are not built)");
    if (p->s.n_agents != p->s.n_total)
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_plan_set_mission_obstacles: a table per mission needs every agent on this device (n_agents == n_total): a sharded plan shares one table");
    if (n_missions != p->n_missions())
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, (std::string(what) + ": " + std::to_string(n_missions) + " obstacle tables for " + std::to_string(p->n_missions()) +
                                                             " missions: one table per mission of the partition in force required (lscqp_plan_set_missions first)").c_str());
    if (p->rec.log_capacity > 0)
        return lscqp_set_error_(LSCQP_ERR_UNSUPPORTED, "lscqp_plan_set_mission_obstacles: the plan has a flight log (lscqp_plan_set_flight_log), whose obstacle columns are those of one shared table");
    int32_t n_slot = 0;
    {   // the offsets: the device entries' own check, by the total the list itself gives once it is known not to decrease
        for (int32_t k = 0; k < n_missions; k++)
            if (obstacle_offsets[k + 1] < obstacle_offsets[k]) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "obstacle_offsets must not decrease");
        PLAN_TRY(lscobstacle::check_obstacle_offsets(p->h, n_missions, obstacle_offsets, obstacle_offsets[n_missions], &n_slot));
    }
    if (n_slot > p->s.n_obs)
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_plan_set_mission_obstacles: a mission's obstacle count exceeds the plan's row slots per agent (max_k count_k <= desc.n_obs required)");
    const int32_t n_dyn = obstacle_offsets[n_missions];
    std::vector<lscqp_obstacle_model> prepared(models, models + n_dyn);
    PLAN_TRY(lscqp_obstacle_model_prepare(prepared.data(), n_dyn));
    return set_obstacle_tables(p, what, param, n_missions, obstacle_offsets, prepared, true);
}

int lscqp_plan_set_obstacle_drives(lscqp_plan p, const lscqp_obstacle_drive* drives, int32_t n_dyn, const double* acc_history, int32_t n_history) {
    if (!p) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null plan");
    if (n_dyn < 0 || n_history < 0) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_plan_set_obstacle_drives: negative size");
    const bool none = n_dyn == 0 || !drives;
    if (!none) {
        if (p->obs.n_dyn == 0)
            return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_plan_set_obstacle_drives: the plan has no obstacles (lscqp_plan_set_obstacles first)");
        if (n_dyn != p->obs.n_dyn)
            return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_plan_set_obstacle_drives: n_dyn is not the number of the plan's obstacles");
        if (n_history > 0 && !acc_history) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_plan_set_obstacle_drives: null acc_history");
        PLAN_TRY(lscqp_obstacle_drive_check(p->obs.models.data(), drives, n_dyn, n_history, p->s.n_total));
        if (p->obs.per_mission) PLAN_TRY(check_chasers_stay_home(p->obs, drives, mission_offsets_of(p)));
    }
    OnDevice on(p->device);
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "lscqp_plan_set_obstacle_drives");
    lscqp_plan_s::Obstacles::Drives next;  // (none: empty)
    if (!none) {  // (everything that can fail comes before the plan changes)
        const size_t nd = (size_t)n_dyn, nh = (size_t)n_history;
        const char* const what = "lscqp_plan_set_obstacle_drives";
        PLAN_TRY(lscqp::dev_alloc(next.d_drives, nd, what));
        PLAN_TRY(lscqp::dev_alloc(next.history, (nh ? nh : 1) * 3, what));
        PLAN_TRY(lscqp::dev_alloc(next.state, nd, what, true));
        e = hipMemcpy(next.d_drives.get(), drives, nd * sizeof(lscqp_obstacle_drive), hipMemcpyHostToDevice);
        if (e == hipSuccess && nh) e = hipMemcpy(next.history.get(), acc_history, nh * 3 * sizeof(double), hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_fail(e, what);
        next.n_history = n_history;
        if (p->obs.per_mission) next.host.assign(drives, drives + nd);  // (the reset asks again where each chaser's target flies)
    }
    drop_graph(p);  // (a captured chain has, or lacks, the drive's node)
    p->obs.drv = std::move(next);
    p->pending = none ? p->pending & ~lscplan::kPendDrives : p->pending | lscplan::kPendDrives;
    return LSCQP_OK;
}

int lscqp_plan_set_patrol(lscqp_plan p, const lscqp_patrol_desc* desc) {
    if (!p) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null plan");
    if (desc) PLAN_TRY(lscqp_patrol_check(desc, p->s.n_agents, p->s.n_total));
    OnDevice on(p->device);
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "lscqp_plan_set_patrol");
    lscqp_plan_s::Patrol next;  // (none: empty)
    if (desc) {  // (everything that can fail comes before the plan changes)
        const size_t nt = (size_t)p->s.n_total;
        const char* const what = "lscqp_plan_set_patrol";
        PLAN_TRY(lscqp::dev_alloc(next.legs, nt, what, true));
        PLAN_TRY(lscqp::dev_alloc(next.swapped, nt, what, true));
        if (p->wp.grid) {  // the plan's own desired goals and start points, and the opposite leg's fields
            next.desired = (double*)p->buf[LSCQP_PLAN_BUF_DESIRED_GOAL], next.start = p->wp.start_pts;
            PLAN_TRY(lscqp::dev_alloc(next.field_other, nt * p->wp.field_nodes, what));
            PLAN_TRY(lscqp::dev_alloc(next.init_d_other, nt, what, true));
        } else {
            PLAN_TRY(lscqp::dev_alloc(next.own_start, nt * 3, what, true));
            if (p->d.optimize_goal) PLAN_TRY(lscqp::dev_alloc(next.own_desired, nt * 3, what, true));
            // static goals: LSCQP_PLAN_BUF_GOAL is the desired goal (goalPlanningWithStaticGoal); with the goal LP it is the LP's to write
            next.desired = p->d.optimize_goal ? next.own_desired.get() : (double*)p->buf[LSCQP_PLAN_BUF_GOAL];
            next.start = next.own_start.get();
        }
        next.desc = *desc;
        next.on = true;
    }
    drop_graph(p);  // (a captured chain has, or lacks, the patrol's nodes)
    p->pat = std::move(next);
    p->wp.fields_valid = false;  // (the agents may be on any leg: the reset puts them on leg 0 and makes the fields of both)
    p->pending |= lscplan::kPendPatrol;
    return LSCQP_OK;
}

void* lscqp_plan_patrol_buffer(lscqp_plan p, int32_t which, uint64_t* bytes_out) {
    if (bytes_out) *bytes_out = 0;
    if (!p || which < 0 || which >= LSCQP_PATROL_COUNT) {
        lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "unknown patrol buffer");
        return nullptr;
    }
    const lscqp_plan_s::Patrol& pat = p->pat;
    if (!pat.on) return nullptr;
    const uint64_t nt = (uint64_t)p->s.n_total, nodes = (uint64_t)p->wp.field_nodes;
    const bool grid = p->wp.grid != nullptr;
    void* q = nullptr;
    uint64_t b = 0;
    switch (which) {
    case LSCQP_PATROL_DESIRED: q = pat.desired, b = nt * 3 * sizeof(double); break;
    case LSCQP_PATROL_START: q = pat.start, b = nt * 3 * sizeof(double); break;
    case LSCQP_PATROL_LEGS: q = pat.legs.get(), b = nt * sizeof(int32_t); break;
    case LSCQP_PATROL_SWAPPED: q = pat.swapped.get(), b = nt * sizeof(int32_t); break;
    case LSCQP_PATROL_FIELD: if (grid) q = p->wp.field.get(), b = nt * nodes * sizeof(int32_t); break;
    case LSCQP_PATROL_INIT_D: if (grid) q = p->wp.init_d, b = nt * sizeof(int32_t); break;
    case LSCQP_PATROL_FIELD_OTHER: if (grid) q = pat.field_other.get(), b = nt * nodes * sizeof(int32_t); break;
    default: if (grid) q = pat.init_d_other.get(), b = nt * sizeof(int32_t); break;
    }
    if (bytes_out) *bytes_out = b;
    return q;
}

namespace {
void* obstacle_buffer(lscqp_plan_s* p, int32_t which, size_t* bytes) {
    *bytes = 0;
    const lscqp_plan_s::Obstacles& o = p->obs;
    if (o.n_dyn == 0) return nullptr;
    switch (which) {
    case LSCQP_PLAN_OBS_TABLE: *bytes = (size_t)o.n_dyn * sizeof(lscqp_obstacle); return o.table.get();
    case LSCQP_PLAN_OBS_SAFETY: *bytes = (size_t)p->s.n_agents * sizeof(lscqp_safety_obs); return o.safety.get();
    case LSCQP_PLAN_OBS_CLOCK: *bytes = (size_t)o.n_tables * sizeof(int32_t); return o.clock.get();
    }
    return nullptr;
}
}  // namespace

void* lscqp_plan_obstacle_buffer(lscqp_plan p, int32_t which, uint64_t* bytes_out) {
    if (bytes_out) *bytes_out = 0;
    if (!p || which < 0 || which >= LSCQP_PLAN_OBS_COUNT) {
        lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "unknown obstacle buffer");
        return nullptr;
    }
    size_t b = 0;
    void* q = obstacle_buffer(p, which, &b);
    if (bytes_out) *bytes_out = b;
    return q;
}

int lscqp_plan_obstacle_upload(lscqp_plan p, int32_t which, const void* host, uint64_t offset, uint64_t bytes) {
    if (!p || !host || which < 0 || which >= LSCQP_PLAN_OBS_COUNT) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "bad argument");
    size_t b = 0;
    void* q = obstacle_buffer(p, which, &b);
    if (offset > b || bytes > b - offset) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "range exceeds the buffer");
    if (bytes == 0) return LSCQP_OK;
    OnDevice on(p->device);
    const hipError_t e = hipMemcpy((char*)q + offset, host, bytes, hipMemcpyHostToDevice);
    return e == hipSuccess ? LSCQP_OK : hip_fail(e, "plan obstacle upload");
}

int lscqp_plan_obstacle_download(lscqp_plan p, int32_t which, void* host, uint64_t offset, uint64_t bytes) {
    if (!p || !host || which < 0 || which >= LSCQP_PLAN_OBS_COUNT) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "bad argument");
    size_t b = 0;
    void* q = obstacle_buffer(p, which, &b);
    if (offset > b || bytes > b - offset) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "range exceeds the buffer");
    if (bytes == 0) return LSCQP_OK;
    OnDevice on(p->device);
    const hipError_t e = hipMemcpy(host, (const char*)q + offset, bytes, hipMemcpyDeviceToHost);  // waits for the device
    return e == hipSuccess ? LSCQP_OK : hip_fail(e, "plan obstacle download");
}

int lscqp_plan_run(lscqp_plan p, int64_t max_replans, int32_t check_every, int32_t use_graph, void* stream, int64_t* replans_enqueued) {
    if (replans_enqueued) *replans_enqueued = 0;
    if (!p) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null plan");
    if (!p->rec.on) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_plan_run: the plan has no record (lscqp_plan_set_record): nothing tells when a mission is over");
    if (!p->d.closed_loop || !p->wp.grid)
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT,
                                "lscqp_plan_run: closed_loop != 0 and waypoint_mode = LSCQP_WAYPOINT_GRID_PIBT required (nothing else flies without host writes between replans)");
    if (max_replans < 1 || check_every < 1) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_plan_run: max_replans >= 1 and check_every >= 1 required");
    int64_t done = 0;
    while (done < max_replans) {
        for (int32_t i = 0; i < check_every && done < max_replans; i++, done++) {
            const int rc = use_graph ? lscqp_plan_step_graph(p, stream) : lscqp_plan_step(p, stream);
            if (replans_enqueued) *replans_enqueued = done;
            if (rc != LSCQP_OK) return rc;
        }
        if (replans_enqueued) *replans_enqueued = done;
        int32_t left = 0;
        OnDevice on(p->device);
        PLAN_TRY(lscqp_record_unfinished_on_(p->rec.held.get(), stream, &left));
        if (left == 0) break;
    }
    return LSCQP_OK;
}

const lscqp_plan_desc* lscqp_plan_desc_of_(lscqp_plan p) { return &p->d; }
int lscqp_plan_device_(lscqp_plan p) { return p->device; }

int64_t lscqp_plan_graph_nodes(lscqp_plan p) {
    if (!p || !p->graph) return 0;
    size_t n = 0;
    if (hipGraphGetNodes(p->graph, nullptr, &n) != hipSuccess) return -1;
    return (int64_t)n;
}

}  // extern "C"
