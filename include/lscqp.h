/*
 * lscqp.h — C ABI of the MI355X-native batched trajectory-QP solver.
 *
 * This is the drop-in boundary for the ONE hot path of qwerty35/lsc_dr_planner:
 * the per-agent, per-replan trajectory QP that the reference builds in
 * TrajOptimizer::populatebyrow (src/traj_optimizer.cpp:216-514) and solves with
 * CPLEX in TrajOptimizer::solve (src/traj_optimizer.cpp:18-156).
 *
 * The reference has no FFI of its own (everything is one statically linked C++
 * executable), so the boundary is a C++ class surface.  The C++ shim in
 * lsc_dr_planner_amd/shim/ keeps that surface (TrajOptimizer /
 * CollisionConstraints / Trajectory, namespace DynamicPlanning) and calls the
 * entry points below; nothing but plain pointers and sizes crosses this ABI.
 *
 * Each entry point cites the reference interface it replaces.
 *
 * Conventions
 *   P  = M*(n+1) control points per axis, n = 5, phi = 3 (the only values the
 *        reference supports, src/traj_optimizer.cpp:184-201).
 *   nv = dim*P decision variables, index x[k*P + m*(n+1) + i]  (axis-major, then
 *        segment, then control point — src/traj_optimizer.cpp:55-57,220-221,241).
 *   All floating-point payloads are fp64.  Inputs that are float32 in the
 *   reference (octomap::point3d) are widened by the caller.
 */
#ifndef LSCQP_H
#define LSCQP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSCQP_VERSION_MAJOR 0
#define LSCQP_VERSION_MINOR 8

/* ---- return codes of the API calls themselves (misuse / runtime errors) ---- */
enum {
    LSCQP_OK = 0,
    LSCQP_ERR_INVALID_ARGUMENT = 1, /* mirrors std::invalid_argument in the reference ctor
                                       (src/traj_optimizer.cpp:200) and populatebyrow (:249) */
    LSCQP_ERR_UNSUPPORTED = 2,      /* class shape has no compiled kernel instance */
    LSCQP_ERR_NO_DEVICE = 3,        /* no HIP device / HIP runtime error: the product path has
                                       no CPU fallback and fails loudly */
    LSCQP_ERR_HIP = 4
};

/* ---- per-instance solve status (status_out[]) ----
 * The reference signals every non-success as `throw PlanningReport::QPFAILED`
 * (src/traj_optimizer.cpp:143,152); the shim maps status != OPTIMAL to that throw. */
enum {
    LSCQP_STATUS_OPTIMAL = 0,
    LSCQP_STATUS_INFEASIBLE = 1, /* CPLEX Infeasible / InfeasibleOrUnbounded, :105-106 */
    LSCQP_STATUS_ITER_LIMIT = 2,
    LSCQP_STATUS_NUMERIC = 3,
    LSCQP_STATUS_CAPACITY = 4    /* hdr.n_obs exceeds the row capacity of the kernel instance the launch selected (n_obs_max too
                                    small, or no compiled instance that large): the instance is REFUSED -- LSC rows are never
                                    dropped silently, the reference gives every obstacle its rows (:399-437) */
};

/* PlannerMode values the QP reads (include/sp_const.hpp:19-26).  Only LSC adds the
 * end-of-horizon stop rows (src/traj_optimizer.cpp:502-511). */
enum {
    LSCQP_PLANNER_DLSC = 0,
    LSCQP_PLANNER_LSC = 1,
    LSCQP_PLANNER_BVC = 2,
    LSCQP_PLANNER_RSFC = 3 /* RECIPROCALRSFC: no end-stop rows, and the z variables of segment 0 are bounded by +-100 instead of the
                              world box (src/traj_optimizer.cpp:255-258).  That planner runs with slack_mode COLLISIONCONSTRAINT:
                              every LSC row then carries a slack in (-inf, 0] that appears in no cost term (:272-283, 423-425), i.e.
                              no LSC row can bind -- callers pass n_obs = 0 (the shim does) */
};

/* Problem class: everything TrajOptimizer caches from Param/Mission at construction
 * (src/traj_optimizer.cpp:4-16) plus the Param fields populatebyrow reads. */
/* Storage format of the packed LSC rows, a property of the class (row_format below).  The reference's LSC record holds its
 * normal and obstacle point as float32 and only d as double (include/collision_constraints.hpp:19-33); LSCQP_ROWS_F32 stores
 * the packed row (nx, ny, nz, b = d + n.p_obs) as four floats -- half the HBM bytes of the batch, SURVEY.md section 8d's byte model
 * for BASELINE configs[4] (10 832 B per QP at M = 5, 20 neighbours; the SFC boxes stay fp64) -- and is widened to fp64 when a kernel stages it: every
 * entry point that reads or writes rows (solve, goal LP, constraint generation) follows the handle's format, the arithmetic
 * stays fp64, and a solve on f32 rows equals bit for bit the solve on f64 rows holding the same float values. */
#define LSCQP_ROWS_F64 0
#define LSCQP_ROWS_F32 1

typedef struct lscqp_class_desc {
    int32_t M;            /* param.M   — number of segments, >= 2 */
    int32_t n;            /* param.n   — must be 5 */
    int32_t phi;          /* param.phi — must be 3 */
    int32_t phi_n;        /* param.phi_n — must be 1 */
    int32_t dim;          /* param.world_dimension, 2 or 3 */
    int32_t planner_mode; /* LSCQP_PLANNER_* */
    int32_t use_sfc;      /* param.world_use_octomap: SFC rows present (:372) */
    int32_t row_format;   /* LSCQP_ROWS_F64 (0, default): lscqp_row, 32 B; LSCQP_ROWS_F32: lscqp_row_f32, 16 B (see below) */
    double dt;                   /* param.dt */
    double control_input_weight; /* param.control_input_weight (:294) */
    double terminal_weight;      /* param.terminal_weight (:304) */
    double communication_range;  /* param.communication_range; <= 0 disables rows (:478) */
    double world_min[3];         /* mission.world_min — variable lower bounds (:252) */
    double world_max[3];         /* mission.world_max — variable upper bounds (:253) */
    /* solver controls (0 selects the default) */
    int32_t max_iter;  /* default 60 */
    int32_t precision; /* LSCQP_PRECISION_* below */
    double tol;        /* relative duality-gap tolerance, 0 = default 1e-10 */
    int32_t warm_start; /* LSCQP_WARM_* below: how an instance that comes with an initial trajectory is centred */
    int32_t active_set; /* LSCQP_ACTIVE_SET_* below: the dual active-set phase in front of the interior-point kernel (0 = default: on) */
} lscqp_class_desc;

/* The dual active-set phase (round 5).  The QP's Hessian is a constant of the class -- jerk cost and terminal pull never depend on the
 * neighbours -- and a plan's optimum holds few of its rows (none at all for 61 of the 64 QPs of BASELINE configs[1]): a first launch
 * over the batch starts every instance at its unconstrained minimiser (three vectors of a per-class table, no factorisation) and adds
 * the violated rows one at a time (Goldfarb-Idnani; csrc/lscqp_das.hip).  What it finishes is marked LSCQP_INFO_ACTIVE_SET and meets
 * the same bar as an interior-point result (1e-9 m on every row, 1e-9 scaled stationarity, multipliers >= 0, exact complementarity);
 * what it does not finish inside its budget (active rows, steps) -- or cannot judge: dependent active rows, capacity, row systems whose
 * emptiness it cannot prove -- is solved by the interior-point kernel behind it in the same call, on the same stream, exactly as without
 * the phase.  Round 6: two verdicts of the phase are final -- LSCQP_STATUS_INFEASIBLE from the phase itself (LSCQP_INFO_ACTIVE_SET set),
 * and the kernel behind skips the instance.  (1) An empty interval, lo > hi on one control point: exact; res_primal = the largest overlap
 * lo - hi.  (2) A violated row with no step left: its normal lies in the span of the active rows' up to a residual part of relative size
 * sqrt(curv / spp) (curv <= 1e-12 spp, in the metric of the class's inverse Hessian), no multiplier gives way, and the violation exceeds
 * 1e-6 m plus what that residual part could buy over the world box's diameter; res_primal = the violation.  That is a Farkas certificate
 * up to the rounding of curv and the metric: row systems that are empty by less are handed over (LSCQP_DAS_WHY_NO_STEP).
 *   LSCQP_ACTIVE_SET_DEFAULT  on
 *   LSCQP_ACTIVE_SET_OFF      the interior-point kernel alone (rounds 1-4; also: LSCQP_ACTIVE_SET=0 in the environment when the handle is
 *                             CREATED -- the library reads its environment in lscqp_create and nowhere else)
 *   LSCQP_ACTIVE_SET_ONLY     the phase alone: instances it leaves are returned LSCQP_STATUS_ITER_LIMIT (development / tests) */
/* Why the phase left an instance (LSCQP_ACTIVE_SET_ONLY: lscqp_info.res_dual of an instance returned LSCQP_STATUS_ITER_LIMIT holds the code,
 * lscqp_info.gap the steps taken; with the interior-point kernel behind the phase the record is that kernel's). */
#define LSCQP_DAS_WHY_CAPACITY 1       /* more obstacles than the launch's kernels hold: LSCQP_STATUS_CAPACITY is the kernel's to give */
#define LSCQP_DAS_WHY_EMPTY_INTERVAL 2 /* lower bound above upper bound on one control point (an empty corridor / world box) */
#define LSCQP_DAS_WHY_ROWS 3           /* more active rows than the launch's budget */
#define LSCQP_DAS_WHY_STEPS 4          /* more steps than the launch's budget */
#define LSCQP_DAS_WHY_NO_STEP 5        /* no step exists for a violated row: its normal lies in the span of the active rows' and no multiplier
                                          blocks -- the row system has no point (a Farkas certificate up to rounding) */
#define LSCQP_DAS_WHY_PIVOT 6          /* a leaving row's rotation lost its pivot (dependent active rows) */
#define LSCQP_DAS_WHY_VERIFICATION 7   /* stationarity above the bar after the polish */
#define LSCQP_DAS_WHY_MULTIPLIER 8     /* a polished multiplier below zero by more than rounding */
#define LSCQP_ACTIVE_SET_DEFAULT 0
#define LSCQP_ACTIVE_SET_OFF 1
#define LSCQP_ACTIVE_SET_ONLY 2

/* Centring of warm-started instances (x_init given).  Every complementarity product starts at mu0 with the slacks floored at s0.
 *   LSCQP_WARM_DEFAULT  (mu0, s0) = (1e-3, 3 cm): safe whatever the quality of the initial trajectory; the shortest TAIL, which is
 *                       what bounds a small batch (a launch lasts as long as its slowest QP).
 *   LSCQP_WARM_TIGHT    (1e-7, 3 mm): presumes the initial trajectory is close to the optimum with the right rows near their bounds --
 *                       the shifted previous plan of a replanning loop usually is.  An instance whose first step comes out shorter
 *                       than 0.6 returns to the default centring after that iteration.  Fewer iterations on average where the start
 *                       is good (4096 x M5 x 20: 3.1 -> 2.2, +6..15 % QP/s; agents holding position: 7.1 -> 4.8) with a longer tail
 *                       everywhere -- 64 x M5: 0.106 -> 0.129 ms, the M = 10 shapes 10..50 % slower, single instances run to the
 *                       iteration limit and are re-solved by the second pass.  A throughput option, not a default. */
#define LSCQP_WARM_DEFAULT 0
#define LSCQP_WARM_TIGHT 1

/* Arithmetic of the interior-point iteration (lscqp_class_desc.precision).
 *   LSCQP_PRECISION_F64    everything fp64 (default; what the reference's CPLEX call computes in, src/traj_optimizer.cpp:66-70).
 *   LSCQP_PRECISION_MIXED  BASELINE configs[4], "fp32 PDIP with fp64 residual check": the reduced KKT matrix is rounded to
 *                          float32 and factorised / substituted in float32 (half the registers and broadcasts of the dominant
 *                          phase); control points, slacks, multipliers, residuals and every stopping test stay fp64, so an
 *                          accepted point meets exactly the same KKT bar as in fp64 mode -- the float32 directions cost
 *                          iterations (+0.4 on the forest class), never accuracy.  Instances on which the float32
 *                          factorisation breaks down (ill-conditioned final iterations; rare on the forest class, common in
 *                          dense mazes) are re-solved by the fp64 kernel in a second pass over the batch inside the same call
 *                          (no host round trip; lscqp_info.flags & LSCQP_INFO_REPAIRED).  The result format (fp64 control
 *                          points, float32 truncation by the shim as in :71-83) is unchanged.
 *                          Available for the throughput shapes (one wavefront per QP); lscqp_create returns
 *                          LSCQP_ERR_UNSUPPORTED for a shape without a compiled mixed instance. */
#define LSCQP_PRECISION_F64 0
#define LSCQP_PRECISION_MIXED 1

/* A packed row in the LSCQP_ROWS_F32 format; pointers declared `lscqp_row*` below then point at arrays of this type, and row
 * offsets stay in units of rows. */
typedef struct lscqp_row_f32 {
    float nx, ny, nz, b;
} lscqp_row_f32;

/* Per-QP header: the fields of Agent (include/sp_const.hpp:146-160) that populatebyrow reads.
 * Exactly 256 bytes. */
typedef struct lscqp_header {
    double p0[3];             /* agent.current_state.position      (:321) */
    double v0[3];             /* agent.current_state.velocity      (:332) */
    double a0[3];             /* agent.current_state.acceleration  (:338) */
    double goal[3];           /* agent.current_goal_point          (:305-313) */
    double next_waypoint[3];  /* agent.next_waypoint               (:494-497) */
    double vmax[3];           /* agent.max_vel[k]                  (:450) */
    double amax[3];           /* agent.max_acc[k]                  (:466) */
    double radius;            /* agent.radius                      (:484) */
    double nominal_velocity;  /* agent.nominal_velocity            (:533) */
    int32_t n_obs;            /* constraints.getObsSize()          (:219) */
    int32_t terminal_segments;/* getTerminalSegments_old(agent) (:530-538) computed by the caller with the
                                 reference's float32 semantics; <= 0: the solver computes it in fp64 */
    uint32_t reserved[2];
    double pad[7];
} lscqp_header;

/* One packed LSC half-space: the constraint  nx*cx + ny*cy + nz*cz >= b  on one control point.
 * From the reference LSC{obs_control_point p, normal_vector nrm, d}
 * (include/collision_constraints.hpp:19-33; row built at src/traj_optimizer.cpp:413-429):
 *     nrm.(c - p) - d >= 0   <=>   nrm.c >= d + nrm.p =: b.
 * Rows with ||nrm|| < 1e-5 are skipped as in the reference (:409-411).  32 bytes. */
typedef struct lscqp_row {
    double nx, ny, nz, b;
} lscqp_row;

/* One SFC box per segment (Box{box_min, box_max}, include/collision_constraints.hpp:39-46;
 * faces via Box::convertToLSCs, src/collision_constraints.cpp:37-59). 48 bytes. */
typedef struct lscqp_box {
    double bmin[3];
    double bmax[3];
} lscqp_box;

/* Optional per-instance solver diagnostics. 32 bytes. */
#define LSCQP_INFO_FLOOR_ACCEPTED 1 /* OPTIMAL by the fallback rule with the one stated deviation: the iteration broke down / stalled /
                                       hit the limit after a point had met the primal (1e-9 m) and gap tests with its stationarity
                                       residual at the rounding floor (<= 1e-6 relative instead of 1e-8); the returned point IS
                                       that point (LSCQP_INFO_REMEMBERED is set too).  Round 4: no instance of the BASELINE
                                       workloads carries it any more (tests/test_floor_audit.py) */
#define LSCQP_INFO_REPAIRED 2       /* solved by the second pass of the call (fp64 after a mixed-precision breakdown, or the
                                       default start after a warm-started failure); iterations counts both passes */
#define LSCQP_INFO_RECENTRED 4      /* a jammed warm start was re-centred once inside the kernel */
#define LSCQP_INFO_REMEMBERED 8     /* the iteration ended by a breakdown / stall / the limit and the result is the BEST point it had
                                       remembered; without LSCQP_INFO_FLOOR_ACCEPTED that point meets the strict tests (1e-9 m,
                                       1e-8, tol) -- it lacks only the second confirmation an iteration that goes on would give */
#define LSCQP_INFO_SHIFTED 16       /* a factorisation lost a pivot to rounding and was repeated with a diagonal shift of
                                       1e-14 (1e-12) max|K|; residuals and stopping tests are exact whatever the direction */
#define LSCQP_INFO_RESCUED 32       /* solved by the RESCUE pass: the instance had run into the iteration limit (a limit cycle of the
                                       predictor-corrector iteration: one cold DLSC instance in ~30 000 of the stress sweeps) or broken
                                       down numerically, and was re-solved on the run-time-shaped kernel with the corrector's
                                       second-order term weighted by the affine step length where that step is blocked (< 0.3) in
                                       the feasible phase.  Run by the host-pointer entries for batches that still hold such an
                                       instance after their other passes, and by retry == 2 of the device entries. */
#define LSCQP_INFO_ACTIVE_SET 64    /* solved by the DUAL ACTIVE SET phase (round 5, csrc/lscqp_das.hip) that runs in front of the interior-point
                                       kernel: Goldfarb-Idnani from the unconstrained minimiser on the class's tabulated inverse.
                                       `iterations` then counts its steps (rows added + rows dropped; 0 = the unconstrained minimiser
                                       violates no row), res_primal is the largest violation over EVERY row at the returned point
                                       (<= 1e-9 m), res_dual the reduced stationarity residual on the interior-point kernel's scale
                                       (verified <= 1e-9), gap is 0: complementarity is exact.  See lscqp_class_desc.active_set. */
typedef struct lscqp_info {
    int32_t iterations;
    int32_t flags;     /* LSCQP_INFO_* */
    double res_primal; /* max inequality violation, metres */
    double res_dual;   /* inf-norm of the reduced stationarity residual, scaled */
    double gap;        /* complementarity: mean s*lambda, scaled */
} lscqp_info;

typedef struct lscqp_solver* lscqp_handle;

/* Replaces TrajOptimizer::TrajOptimizer (src/traj_optimizer.cpp:4-16): validates (n,phi)==(5,3) like
 * buildAeqBase (:198-201), precomputes Q_base (:163-178) and the continuity structure (:180-214),
 * uploads class constants to the device. */
int lscqp_create(const lscqp_class_desc* desc, lscqp_handle* out);

/* Replaces TrajOptimizer::updateParam (src/traj_optimizer.cpp:158-160): re-derive class constants.  Launches already enqueued (or captured
 * in a graph) keep the constants they were enqueued with: the class travels by value in kernel arguments, and the active-set tables of a
 * device are immutable once a launch may have seen them -- an update that changes them (dt, weights, M, planner mode, communication range
 * on/off) gives every device that holds a copy a FRESH buffer and retires the old one; the reference's own updates (slack_mode flips,
 * src/traj_planner.cpp:155,160,187,214) change none of these and touch nothing on the device.  Not a device synchronisation point. */
int lscqp_update(lscqp_handle h, const lscqp_class_desc* desc);

/* The class's active-set tables on the CURRENT device, now.  lscqp_create loads them on the device that is current then; any other device's
 * first solve loads them lazily -- which a launch inside a stream capture cannot do (hipMalloc / hipMemcpy are not allowed there): such a
 * launch returns LSCQP_ERR_HIP and names this function, instead of silently running without the phase.  lscqp_comm_prepare does it for every
 * device of a communicator. */
int lscqp_prepare_device(lscqp_handle h);

int lscqp_destroy(lscqp_handle h);

/* nv = dim*M*(n+1): number of doubles per instance in x_out. */
int lscqp_num_variables(lscqp_handle h);
/* M, whether the class carries SFC rows, and the bytes of one packed row in the handle's row_format (32 or 16). */
int lscqp_num_segments(lscqp_handle h);
/* The largest number of obstacles per agent any compiled kernel instance of the handle's shape and precision holds: the n_obs_max
 * beyond which lscqp_solve_batch_device returns LSCQP_ERR_UNSUPPORTED.  A caller that must not drop neighbours (the reference
 * never does, src/multi_sync_simulator.cpp:318-333) sizes its row buffers from lscqp_select_neighbours_device's in-range counts,
 * up to this bound. */
int lscqp_max_obstacles(lscqp_handle h);
int lscqp_uses_sfc(lscqp_handle h);
int lscqp_row_bytes(lscqp_handle h);

/* Replaces TrajOptimizer::solve (src/traj_optimizer.cpp:18-156) for a batch of n independent agents
 * (the sequential loop at src/multi_sync_simulator.cpp:354-362 issues n == 1).
 * HOST pointers; synchronous; copies in, launches the HIP kernel, copies out.
 *   hdr          [n]
 *   rows         packed LSC rows; instance q owns rows[row_offsets[q] .. row_offsets[q] + hdr[q].n_obs*P),
 *                ordered [oi][m][i] exactly like CollisionConstraints::lscs (include/collision_constraints.hpp:173)
 *                (the m==0,i<3 entries are present and ignored, :404-406)
 *   row_offsets  [n+1] in units of rows (uint64)
 *   sfc          [n*M] boxes, or NULL when !use_sfc
 *   x_init       [n*nv] or NULL: the `initial_traj` argument of TrajOptimizer::solve (the shifted previous plan,
 *                src/traj_planner.cpp:399-411) as control points in the reference variable order.  CPLEX ignores it
 *                (src/traj_optimizer.cpp:516-528 is dead code); here it is the primal start of the interior-point
 *                iteration (same optimum, about one iteration fewer in steady state).  NULL: start from hover.
 *   x_out        [n*nv]  raw fp64 control points, reference variable order (no float32 truncation)
 *   obj_out      [n]     objective INCLUDING the constant terminal term, == cplex.getObjValue() (:100)
 *   status_out   [n]     LSCQP_STATUS_*
 *   info_out     [n] or NULL
 * An iteration started from the caller's trajectory can jam against the boundary (a few instances per ten thousand); the
 * kernel re-centres such an instance once.  With x_init given, instances that still end in ITER_LIMIT / NUMERIC are solved
 * once more from the default start before this call returns (lscqp_info.iterations then counts both attempts); the device
 * variant below cannot look at the statuses without synchronising and leaves that to its caller. */
int lscqp_solve_batch(lscqp_handle h, int64_t n, const lscqp_header* hdr, const lscqp_row* rows,
                      const uint64_t* row_offsets, const lscqp_box* sfc, const double* x_init, double* x_out,
                      double* obj_out, int32_t* status_out, lscqp_info* info_out);

/* lscqp_solve_batch with the H2D copy, the kernels and the D2H copy issued on the CALLER's stream (a hipStream_t passed as
 * void*; NULL = a private non-blocking stream of the call); returns after that stream has been synchronised.
 * THREAD SAFETY of the host-pointer entry points (this one, lscqp_solve_batch, lscqp_optimize_goal, lscqp_construct_sfc): each
 * call stages through its own (device buffer, pinned mirror, stream) slot taken from a pool inside the handle, so any number of
 * threads may call them concurrently on the same solver / map handle -- the reference builds a fresh IloEnv per call and is
 * re-entrant in the same sense (src/traj_optimizer.cpp:25-29).  lscqp_update / lscqp_destroy must not race with calls in flight. */
int lscqp_solve_batch_stream(lscqp_handle h, int64_t n, const lscqp_header* hdr, const lscqp_row* rows,
                             const uint64_t* row_offsets, const lscqp_box* sfc, const double* x_init, double* x_out,
                             double* obj_out, int32_t* status_out, lscqp_info* info_out, void* stream);

/* Same, DEVICE pointers, asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream).
 * Inputs must already be resident in HBM; nothing is copied and nothing is synchronised.
 * n_obs_max: upper bound of d_hdr[q].n_obs over the batch; it selects the kernel instance (row slots in registers, LDS
 * staging area).  An instance whose n_obs exceeds the selected kernel's capacity is refused with LSCQP_STATUS_CAPACITY --
 * rows are never dropped -- so pass the true maximum; LSCQP_ERR_UNSUPPORTED if no compiled instance holds n_obs_max.
 * retry != 0: a second pass over the batch on the same stream re-solves, from the default start, the instances that the
 * first pass did not bring to OPTIMAL (jammed / diverged warm starts; what lscqp_solve_batch does for its callers) --
 * no host round trip, ~3 us when there is nothing to repair.  retry == 2: the second pass runs on the compiled instance that
 * eliminates the reduced system in the OTHER order (natural vs nested dissection; M = 10 in 2-D has both), also for batches
 * without a start trajectory -- a factorisation that breaks down in one order usually survives in the other; that instance costs
 * ~35 us to launch even with nothing to repair, so it is not what retry == 1 does.  retry == 2 also ends with the RESCUE pass
 * (LSCQP_INFO_RESCUED: instances still at the iteration limit / a numerical breakdown, on the run-time-shaped kernel with a weighted
 * corrector).  retry == 3: the second pass from the default start AND the rescue pass, without the other-order pass -- two launches that
 * return at once for every instance already OPTIMAL (each tests the status before it fetches anything); what lscqp_plan's chain enqueues
 * in every replan (the reference tries a failed QP again on the spot, src/traj_planner.cpp:763-766).  Other values: LSCQP_ERR_INVALID_ARGUMENT.
 * The host-pointer entries run both by themselves, and only for batches that still hold such an instance after the first call.
 * In LSCQP_PRECISION_MIXED the fp64 second pass always runs. */
int lscqp_solve_batch_device_ex(lscqp_handle h, int64_t n, int32_t n_obs_max, const lscqp_header* d_hdr,
                                const lscqp_row* d_rows, const uint64_t* d_row_offsets, const lscqp_box* d_sfc,
                                const double* d_x_init, double* d_x_out, double* d_obj_out, int32_t* d_status_out,
                                lscqp_info* d_info_out, int32_t retry, void* stream);
/* lscqp_solve_batch_device_ex with retry = 0. */
int lscqp_solve_batch_device(lscqp_handle h, int64_t n, int32_t n_obs_max, const lscqp_header* d_hdr,
                             const lscqp_row* d_rows, const uint64_t* d_row_offsets, const lscqp_box* d_sfc,
                             const double* d_x_init, double* d_x_out, double* d_obj_out, int32_t* d_status_out,
                             lscqp_info* d_info_out, void* stream);

/* Work order of a launch (round 4).  A launch with more instances than the chip holds at once is run by PERSISTENT workgroups that take
 * instance after instance from a queue (list scheduling; nothing to ask for, lscqp_solve_batch_device[_ex] do it by themselves).  The
 * launch then lasts sum / slots + (what is still running when the queue is empty): starting the LONGEST instances first shortens that
 * tail -- 1024 x M10 x 40 on one MI355X: 1.14 ms in the given order with one instance per workgroup, see DESIGN.md section 4 for the
 * figures with the queue and with the order.  The iteration count of the previous replan's solve of the same agent is the hint a
 * planner has (lscqp_plan carries it from replan to replan by itself when its QP launch exceeds lscqp_launch_capacity):
 *   lscqp_order_by_work_device   d_order_out[n] := the instances sorted by d_info_prev[i].iterations, most first, ties in index order
 *   lscqp_solve_batch_device_ordered   lscqp_solve_batch_device_ex with the k-th slot of the launch solving instance d_order[k]
 *                                (a permutation of 0 .. n-1; NULL = identity).  Results land at the instance's own index, bit for bit
 *                                what any other order gives.  The permutation is trusted; a handle created with LSCQP_CHECK_ORDER=1
 *                                in the environment verifies it on the device in every call first (an allocation and a synchronisation:
 *                                a debugging aid) and returns LSCQP_ERR_INVALID_ARGUMENT for a stale or short order buffer. */
/* instances of a launch of n the device works on at once (CUs x workgroups per CU of the kernel instance the launch selects); a launch of
 * more runs in rounds and has a tail -- that is where the order pays.  -1 without a device. */
int64_t lscqp_launch_capacity(lscqp_handle h, int64_t n, int32_t n_obs_max);
/* instances ONE device works on at once in the kernel that carries a solve of this class: the dual active-set phase's resident workgroups
 * when the phase is on AND finishing what it is given; lscqp_launch_capacity (the interior-point instance's) when the phase is off or the
 * handle's last host-pointer call had to run the interior-point passes behind it.  -1 without a device. */
int64_t lscqp_device_fill(lscqp_handle h, int64_t n, int32_t n_obs_max);
int lscqp_order_by_work_device(int64_t n, const lscqp_info* d_info_prev, int32_t* d_order_out, void* stream);
int lscqp_solve_batch_device_ordered(lscqp_handle h, int64_t n, int32_t n_obs_max, const lscqp_header* d_hdr, const lscqp_row* d_rows,
                                     const uint64_t* d_row_offsets, const lscqp_box* d_sfc, const double* d_x_init, double* d_x_out,
                                     double* d_obj_out, int32_t* d_status_out, lscqp_info* d_info_out, int32_t retry,
                                     const int32_t* d_order, void* stream);

/* ---- multi-GPU: the agent batch over the GPUs of one node, from ONE host process ----------------
 *
 * The reference's host is a single process (one ROS node); within a replan step its N QPs are independent
 * (src/multi_sync_simulator.cpp:354-362) and the only exchange is broadcastMsgs (:305-352: every agent receives the others'
 * previous plans).  A communicator owns one private stream, one staging pool and one RCCL communicator per device
 * (ncclCommInitAll; RCCL is bound at run time, a single-GPU host needs none).  Partitioning: contiguous blocks of
 * ceil(N / G) agents in id order; NO collective on the solve path.
 *   lscqp_comm_create        n_devices <= 0: all visible devices; device_ids NULL: 0 .. n_devices-1
 *   lscqp_comm_backend       "rccl <version> (ncclCommInitAll, G devices)" or "none: single device, ..." -- what actually runs
 *   lscqp_comm_devices_for   how many devices a batch of n agents is spread over: clamp(n / min_agents_per_device, 1, G), default
 *                            256 agents per device -- one 64-QP block per device finishes no sooner than 512 QPs on one
 *                            device (0.108 vs 0.136 ms at M = 5), so spreading a small batch buys nothing and only adds the
 *                            exchange; north_star: "only when agent count justifies it".  lscqp_comm_set_min_agents_per_device
 *                            moves the threshold (1 = always use every device).
 *   lscqp_comm_devices_for_class   the rule lscqp_solve_batch_sharded applies (round 5), with the class in hand: clamp(n / fill, 1, G),
 *                            fill = lscqp_device_fill(h, n, n_obs_max) = the instances ONE device works on at once in the first
 *                            kernel of a solve (the dual active-set phase's resident workgroups, or lscqp_launch_capacity without
 *                            the phase, or while the phase keeps leaving work to the slower kernel): a second device is used only
 *                            where one would need a second round.  A threshold set with lscqp_comm_set_min_agents_per_device
 *                            overrides it.  THE rule of the library: lscqp_solve_batch_sharded applies it, and a caller of
 *                            lscqp_solve_batch_sharded_device (who cuts the blocks himself) asks it here; lscqp_comm_devices_for is
 *                            its class-free fallback for callers without a handle.
 *   lscqp_comm_prepare       the class's active-set tables on every device of the communicator, now (a device's first solve loads
 *                            them lazily otherwise -- which a launch inside a stream capture cannot do: it fails, loudly)
 *   lscqp_comm_shard         the block [first, first + count) of device g when n agents are spread over n_used devices
 *   lscqp_solve_batch_sharded        HOST pointers for the whole batch (same arguments as lscqp_solve_batch): every block is staged
 *                            to its device, solved there (with the retry pass) and fetched back, all devices concurrently, each
 *                            on its own stream; results land in the caller's arrays in agent order.  *n_devices_used reports the
 *                            spread.  This is what TrajOptimizer::solveBatch calls when it has a communicator.
 *   lscqp_solve_batch_sharded_device DEVICE-resident blocks: arrays of G per-device pointers, n[g] agents on device g, launched on
 *                            the communicator's streams, asynchronous (lscqp_comm_synchronize waits for all of them)
 *   lscqp_allgather          the device analogue of broadcastMsgs: device g contributes d_send[g][count] doubles (its block of
 *                            solved control points, x_out) and receives everybody's into d_recv[g][G * count]; one grouped
 *                            ncclAllGather over xGMI on the communicator's streams, asynchronous.  Equal counts per device:
 *                            pad the last block.  count * 8 B per device is 46 KB (64 agents, M = 5) to 369 KB (512 agents):
 *                            latency-bound on xGMI, hence the spreading rule above. */
typedef struct lscqp_comm_s* lscqp_comm;
int lscqp_comm_create(int32_t n_devices, const int32_t* device_ids, lscqp_comm* out);
void lscqp_comm_destroy(lscqp_comm c);
int32_t lscqp_comm_size(lscqp_comm c);
int32_t lscqp_comm_device(lscqp_comm c, int32_t g);
void* lscqp_comm_stream(lscqp_comm c, int32_t g); /* hipStream_t of device g */
const char* lscqp_comm_backend(lscqp_comm c);
int lscqp_comm_set_min_agents_per_device(lscqp_comm c, int64_t n);
int32_t lscqp_comm_devices_for(lscqp_comm c, int64_t n);
int32_t lscqp_comm_devices_for_class(lscqp_comm c, lscqp_handle h, int64_t n, int32_t n_obs_max);
int lscqp_comm_prepare(lscqp_comm c, lscqp_handle h);
int lscqp_comm_shard(lscqp_comm c, int64_t n, int32_t n_used, int32_t g, int64_t* first, int64_t* count);
/* the same partition rule without a communicator (no device needed): block g of n agents over n_used devices */
int lscqp_shard_range(int64_t n, int32_t n_used, int32_t g, int64_t* first, int64_t* count);
int lscqp_comm_synchronize(lscqp_comm c);
int lscqp_solve_batch_sharded(lscqp_handle h, lscqp_comm c, int64_t n, const lscqp_header* hdr, const lscqp_row* rows,
                              const uint64_t* row_offsets, const lscqp_box* sfc, const double* x_init, double* x_out, double* obj_out,
                              int32_t* status_out, lscqp_info* info_out, int32_t* n_devices_used);
int lscqp_solve_batch_sharded_device(lscqp_handle h, lscqp_comm c, const int64_t* n, int32_t n_obs_max, const lscqp_header* const* d_hdr,
                                     const lscqp_row* const* d_rows, const uint64_t* const* d_row_offsets, const lscqp_box* const* d_sfc,
                                     const double* const* d_x_init, double* const* d_x_out, double* const* d_obj_out,
                                     int32_t* const* d_status_out, lscqp_info* const* d_info_out, int32_t retry);
int lscqp_allgather(lscqp_comm c, const double* const* d_send, double* const* d_recv, int64_t count);
/* The exchange that follows a sharded replan, as a list of collective operations (no device needed: this is the bookkeeping
 * lscqp_plan_group_step executes over RCCL, exported so that it can be checked for any device count on a host without GPUs).
 * Device g owns agents [first[g], first[g] + count[g]) of n_total; the blocks must be consecutive in device order and cover the
 * mission (LSCQP_ERR_INVALID_ARGUMENT otherwise).  Every device holds a buffer of n_total * per doubles in agent order and has
 * just rewritten its own block.  Equal blocks: ONE in-place all-gather (kind LSCQP_XCHG_ALLGATHER: every device sends `count`
 * doubles from `offset_of_device[g] = first[g] * per`, block g lands at first[g] * per on every device).  A short or empty last
 * block: one broadcast per NON-EMPTY owner (kind LSCQP_XCHG_BROADCAST, root = the owner, `offset` / `count` in doubles), empty
 * owners are skipped by every device alike.  Returns the number of operations in *n_ops (<= n_devices).
 *
 * lscqp_exchange_schedule_padded: the same with `pad_agents` agents of room BEHIND the mission in every device's buffer.  The blocks
 * lscqp_shard_range cuts -- ceil(n_total / G) agents each, a shorter one, then empty ones -- start at multiples of the block size, so a
 * ragged mission is ONE in-place all-gather of the full block size as well (device g sends from g * B * per; what a short or empty
 * block sends beyond its agents lands behind the mission, in the padding) whenever G * B - n_total <= pad_agents; otherwise, and for
 * blocks of any other shape, the broadcasts above.  The three buffers lscqp_plan_group_step exchanges (LSCQP_PLAN_BUF_PLAN, _STATE,
 * _GOAL) are allocated with LSCQP_PLAN_EXCHANGE_PAD agents of such room (G * B - n_total < G <= 64 always): a group of plans cut by
 * lscqp_shard_range exchanges with one all-gather per buffer whatever the agent count.  lscqp_plan_buffer keeps reporting the
 * mission's own bytes. */
#define LSCQP_PLAN_EXCHANGE_PAD 64
#define LSCQP_XCHG_ALLGATHER 0
#define LSCQP_XCHG_BROADCAST 1
typedef struct lscqp_exchange_op {
    int32_t kind; /* LSCQP_XCHG_* */
    int32_t root; /* broadcast: the owner; all-gather: -1 */
    int64_t offset; /* doubles from the start of the buffer: broadcast: the owner's block; all-gather: 0 (block g at g * count) */
    int64_t count;  /* doubles: broadcast: the owner's block; all-gather: the (equal) block of every device */
} lscqp_exchange_op;
int lscqp_exchange_schedule(int64_t n_total, int32_t n_devices, const int64_t* first, const int64_t* count, int64_t per,
                            lscqp_exchange_op* ops, int32_t max_ops, int32_t* n_ops);
int lscqp_exchange_schedule_padded(int64_t n_total, int32_t n_devices, const int64_t* first, const int64_t* count, int64_t per, int64_t pad_agents,
                                   lscqp_exchange_op* ops, int32_t max_ops, int32_t* n_ops);

/* ---- next row of the path: the producer of the LSC rows --------------------------------
 *
 * Replaces TrajPlanner::generateLSC for agent-type obstacles (reference src/traj_planner.cpp:611-657), i.e.
 * normalVectorBetweenPolys (:1179-1205), the closest point of closestPointsBetweenPointAndConvexHull
 * (include/geometry.hpp:266-296; openGJK in the reference), downwashBetween (:1229-1240),
 * Trajectory::coordinateTransform (src/trajectory.cpp:207-219) and CollisionConstraints::setLSC
 * (src/collision_constraints.cpp:514-521) -- and writes the result directly in the packed row layout that
 * lscqp_solve_batch_device consumes (rows of local agent a at offset a * n_obs * M * (n+1), order [oi][m][i]).
 * DEVICE pointers, asynchronous on `stream`.
 *   d_traj        [n_total][M][n+1][3]  control points of ALL agents: the planning agent's initial trajectory and a
 *                 neighbour's predicted trajectory are both shifted previous plans (:273-310, 399-411); values as the
 *                 reference holds them (float32-representable; lscqp_shift_traj_device produces exactly this)
 *   d_neighbours  [n_agents][n_obs]     global agent ids of each local agent's obstacles; < 0 = none -> all-zero rows
 *                 (the solver drops them like any normal shorter than 1e-5, src/traj_optimizer.cpp:409-411)
 *   d_radius, d_downwash [n_total]      Agent::radius, Agent::downwash
 *   d_goal        [n_agents][3]         current_goal_point: fallback normal when the hull contains the origin (:624-633)
 *   first_agent   global id of local agent 0 (the local shard is [first_agent, first_agent + n_agents))
 *   d_rows_out    [n_agents * n_obs * M * (n+1)] rows
 * Dynamic (non-agent) obstacles and collision-predicted obstacles (the other branches of generateLSC) are not handled;
 * generateCLSC and generateBVC are served by lscqp_generate_constraints_device below. */
int lscqp_generate_lsc_device(lscqp_handle h, int64_t n_agents, int32_t n_obs, int64_t first_agent, const double* d_traj,
                              const int32_t* d_neighbours, const double* d_radius, const double* d_downwash,
                              const double* d_goal, lscqp_row* d_rows_out, void* stream);

/* The planner's other constraint generators for agent-type obstacles, same inputs / output layout / launch as
 * lscqp_generate_lsc_device, selected by `mode`:
 *   LSCQP_GEN_LSC   generateLSC  (src/traj_planner.cpp:611-657)  -- identical to lscqp_generate_lsc_device
 *   LSCQP_GEN_CLSC  generateCLSC (:659-706): what constructLSC() runs for the reference's default launch (mode/planner = lsc
 *                   with mode/goal = grid_based_planner, :551-553).  Segments m < M-1 as generateLSC without the fallback
 *                   normal (a hull around the origin leaves zero rows); the last segment separates the line segments
 *                   (last control point -> goal point) of the neighbour and of the agent with
 *                   closestPointsBetweenLineSegments (include/geometry.hpp:174-263) and carries one obstacle point and one
 *                   margin for all control points (CollisionConstraints::setLSC, src/collision_constraints.cpp:532-539)
 *   LSCQP_GEN_BVC   generateBVC  (:708-734): buffered Voronoi cell from the two start points
 *   d_goal_all [n_total][3]: current goal point of EVERY agent (the planning agent's own, agent.current_goal_point, and the
 *   neighbours', obstacles[oi].goal_point as broadcast), indexed by global id. */
#define LSCQP_GEN_LSC 0
#define LSCQP_GEN_CLSC 1
#define LSCQP_GEN_BVC 2
int lscqp_generate_constraints_device(lscqp_handle h, int32_t mode, int64_t n_agents, int32_t n_obs, int64_t first_agent,
                                      const double* d_traj, const int32_t* d_neighbours, const double* d_radius,
                                      const double* d_downwash, const double* d_goal_all, lscqp_row* d_rows_out, void* stream);

/* Who is whose obstacle: MultiSyncSimulator::broadcastMsgs (src/multi_sync_simulator.cpp:305-352) hands agent i every other
 * agent j with LInfinityDistance(p_i, p_j) <= communication_range (include/util.hpp:122-131; all of them if the range is <= 0),
 * in id order.  d_positions [n_total][3]: the agents' current positions (float32 values, all-gathered when sharded).
 * d_neighbours_out [n_agents][n_obs]: the global ids in ascending order, padded with -1 -- the list
 * lscqp_generate_*_device consumes.  The reference's list is unbounded; here the row buffers hold n_obs neighbours per
 * agent, so when more are in range the n_obs NEAREST are kept (L-infinity distance, ties to the smaller id; still listed in
 * id order).  d_count_out [n_agents]: how many were in range (> n_obs tells the caller that the list was cut). */
int lscqp_select_neighbours_device(lscqp_handle h, int64_t n_agents, int64_t first_agent, int64_t n_total, int32_t n_obs,
                                   double communication_range, const double* d_positions, int32_t* d_neighbours_out,
                                   int32_t* d_count_out, void* stream);

/* Replaces TrajPlanner::initialTrajPlanningPrevSol (src/traj_planner.cpp:399-411) on the solver's output: segment m of
 * the new initial trajectory := segment m+1 of the previous plan, the last segment := its last point; control points
 * truncated to float32 like TrajOptResult::desired_traj (src/traj_optimizer.cpp:71-83); dim == 2 -> z := z_2d.
 *   d_x_prev [n][dim*M*(n+1)] (x_out of lscqp_solve_batch_device)  ->  d_traj [n][M][n+1][3]
 *   shift_segments: 1 = the reference's shift; 0 = layout change and truncation only (replanning from the same state) */
int lscqp_shift_traj_device(lscqp_handle h, int64_t n, int32_t shift_segments, double z_2d, const double* d_x_prev,
                            double* d_traj, void* stream);

/* lscqp_generate_constraints_device writing into a row buffer that holds n_obs_total obstacle slots per agent: the n_obs
 * neighbour slots of this call go to slots slot0 .. slot0 + n_obs - 1 of each agent's block (the other slots belong to another
 * producer, e.g. lscqp_generate_lsc_obstacles_device).  n_obs_total = n_obs, slot0 = 0 is lscqp_generate_constraints_device. */
int lscqp_generate_constraints_device_ex(lscqp_handle h, int32_t mode, int64_t n_agents, int32_t n_obs, int64_t first_agent,
                                         const double* d_traj, const int32_t* d_neighbours, const double* d_radius,
                                         const double* d_downwash, const double* d_goal_all, lscqp_row* d_rows_out, int32_t n_obs_total,
                                         int32_t slot0, void* stream);

/* The NON-AGENT branches of TrajPlanner::generateLSC (reference src/traj_planner.cpp:611-657) with what feeds them:
 * constant-velocity prediction of a dynamic obstacle (obstaclePredictionWithPrevSol :283-285, Trajectory::planConstVelTraj,
 * src/trajectory.cpp:79-91), checkObstacleDisturbance (:312-319), obstacleSizePredictionWithConstAcc (:321-358: the obstacle's
 * radius grows with 1/2 max_acc t^2 over the uncertainty horizon, plus a velocity guard of the planning agent), downwashBetween
 * for a non-agent (:1235-1237), the z component of the relative hull dropped for obstacles taller than obs_downwash_threshold
 * (:1188-1191), margin d = predicted size + agent radius (:646-648), and the fallback normal (:624-633).
 * (normalVectorDynamicObs, :1207-1227, is dead code in the reference: col_pred_obs_indices is never filled.)
 *   d_obstacle_ids [n_agents][n_dyn]  index into d_obstacles of each local agent's obstacles, < 0 = none -> all-zero rows
 *   d_obstacles    [..]               the obstacle table (include/obstacle.hpp:13-27, the fields the planner reads)
 *   d_traj         [n_total][M][n+1][3]  initial trajectories (only the local agents' are read), d_radius [n_total]
 *   d_goal         [n_agents][3]      current goal points of the local agents;  d_hdr [n_agents]: v0 and amax[0] (velocity guard)
 *   rows go to slots slot0 .. slot0 + n_dyn - 1 of each agent's block of n_obs_total slots in d_rows_out. */
typedef struct lscqp_obstacle {
    double position[3];
    double velocity[3];
    double radius, downwash, max_acc;
    int32_t type; /* 0 = DYNAMICOBSTACLE, 1 = AGENT (include/sp_const.hpp:135-138) */
    int32_t reserved;
} lscqp_obstacle;
typedef struct lscqp_obstacle_param { /* src/param.cpp:63-67, 106-108 */
    double obs_uncertainty_horizon; /* obs/uncertainty_horizon (1) */
    double velocity_guard_ratio;    /* obs/velocity_guard_ratio (0.75) */
    double obs_downwash_threshold;  /* plan/obs_downwash_threshold (3.0) */
    double reset_threshold;         /* plan/reset_threshold (0.1; 0.5 in the launch files) */
    int32_t obs_size_prediction;    /* obs/size_prediction (true) */
    int32_t use_velocity_guard;     /* obs/use_velocity_guard (true) */
} lscqp_obstacle_param;
int lscqp_generate_lsc_obstacles_device(lscqp_handle h, const lscqp_obstacle_param* param, int64_t n_agents, int32_t n_dyn,
                                        int64_t first_agent, const double* d_traj, const int32_t* d_obstacle_ids,
                                        const lscqp_obstacle* d_obstacles, const double* d_radius, const double* d_goal,
                                        const lscqp_header* d_hdr, lscqp_row* d_rows_out, int32_t n_obs_total, int32_t slot0, void* stream);

/* The rows of non-agent obstacles for the constraint generator constructLSC selects (:551-557), same units, slot remap and row formats as
 * lscqp_generate_lsc_obstacles_device, selected by `mode`:
 *   LSCQP_GEN_LSC   lscqp_generate_lsc_obstacles_device itself, argument for argument (the same bits); d_obstacle_goal is ignored
 *   LSCQP_GEN_CLSC  the non-agent branch of generateCLSC (:659-706): an in-range agent and a dynamic obstacle are treated alike.  Segments
 *                   m < M-1: the normal of normalVectorBetweenPolys between the agent's initial trajectory and the obstacle's
 *                   constant-velocity prediction (z of the hull dropped for a tall dynamic obstacle, :1188-1191; no fallback normal: a hull
 *                   around the origin leaves zero rows) and the reciprocal half margin d_i = (radius + r_own + rel_i . n) / 2 -- against an
 *                   obstacle that does not do its half, so a CLSC row can let the agent closer than an LSC row would.  Segment M-1: the
 *                   line segments (predicted last point -> obstacle goal point) and (own last point -> agent goal point) separated by
 *                   closestPointsBetweenLineSegments, one obstacle point and one margin for all control points.  downwashBetween for a
 *                   non-agent (:1235-1237), the transform skipped in 2-D (:666-672).  In 2-D the row is the one the 2-D QP and goal LP
 *                   build from the record (src/traj_optimizer.cpp:414-421): n_z = 0 and b = d + n_x p_x + n_y p_y, whatever z the
 *                   record's normal and obstacle point have -- on the last segment they have one when the obstacle's goal point lies
 *                   off the mission's plane, as the origin does at z_2d != 0.  obs_pred_sizes and the velocity guard play no part:
 *                   of `param` only obs_downwash_threshold is read, and d_hdr may be NULL.
 *   LSCQP_GEN_BVC   LSCQP_ERR_UNSUPPORTED (generateBVC's non-agent branch is not built); any other mode LSCQP_ERR_INVALID_ARGUMENT
 *   d_obstacle_goal [..][3]  Obstacle::goal_point per entry of the obstacle table, or NULL = the origin for every obstacle: what the
 *                   reference's ObstacleGenerator::getObstacle leaves there (include/obstacle.hpp:23, 37-49 never set it).  CLSC only. */
int lscqp_generate_obstacle_rows_device(lscqp_handle h, int32_t mode, const lscqp_obstacle_param* param, int64_t n_agents, int32_t n_dyn,
                                        int64_t first_agent, const double* d_traj, const int32_t* d_obstacle_ids,
                                        const lscqp_obstacle* d_obstacles, const double* d_obstacle_goal, const double* d_radius,
                                        const double* d_goal, const lscqp_header* d_hdr, lscqp_row* d_rows_out, int32_t n_obs_total, int32_t slot0,
                                        void* stream);

/* initialTrajPlanningPrevSol / obstaclePredictionWithPrevSol when the simulation step is SHORTER than a segment
 * (multisim_time_step < dt, reference src/traj_planner.cpp:296-306, 413-421): segment 0 of the new initial trajectory :=
 * prev_traj[0].subSegment(fraction, 1) (Segment::subSegment, src/trajectory.cpp:15-49), the other segments are kept.
 * fraction = multisim_time_step / dt in (0, 1); layouts and float32 truncation as lscqp_shift_traj_device. */
int lscqp_shift_traj_partial_device(lscqp_handle h, int64_t n, double fraction, double z_2d, const double* d_x_prev, double* d_traj,
                                    void* stream);

/* Algorithmic HBM bytes of one lscqp_generate_lsc_device call: rows written + every agent's control points,
 * neighbour list, radius, downwash and goal read once. */
int64_t lscqp_generate_lsc_bytes(lscqp_handle h, int64_t n_agents, int32_t n_obs, int64_t n_total);

/* ---- next row of the path: the planner's other CPLEX call -------------------------------
 *
 * Replaces GoalOptimizer::solve (reference src/goal_optimizer.cpp:7-70; model :72-147): the one-variable LP
 *     min t in [0, 1 + 1e-5]   s.t.   n_r . ((g - w) t + w - p_r) - d_r >= 0
 * over the SFC faces of the last segment (if use_sfc) and the LSC rows (oi, M-1, n) of every obstacle, solved in
 * closed form on the device.  On entry hdr[q].goal = current_goal_point g and hdr[q].next_waypoint = w; on return
 * hdr[q].goal = (g - w) t* + w (:55), ready for lscqp_solve_batch*.  rows / row_offsets / sfc exactly as for the solve.
 * status_out[q] = LSCQP_STATUS_OPTIMAL, or LSCQP_STATUS_INFEASIBLE where the reference throws QPFAILED (goal unchanged).
 * |g - w| < 1e-5 returns w like the reference (:12-14). */
int lscqp_optimize_goal_device(lscqp_handle h, int64_t n, lscqp_header* d_hdr, const lscqp_row* d_rows,
                               const uint64_t* d_row_offsets, const lscqp_box* d_sfc, int32_t* d_status_out, void* stream);
/* Same, HOST pointers, synchronous (hdr is updated in place). */
int lscqp_optimize_goal(lscqp_handle h, int64_t n, lscqp_header* hdr, const lscqp_row* rows, const uint64_t* row_offsets,
                        const lscqp_box* sfc, int32_t* status_out);

/* ---- next row of the path: what the planner does with a solved trajectory ----------------
 *
 * Replaces, for a batch, TrajPlanner::isSolValid (reference src/traj_planner.cpp:990-1045: SFC containment of the control
 * points, velocity / acceleration within 1 % of the limits at the simulation step), Trajectory::getStateAt
 * (src/trajectory.cpp:156-170) and AgentManager::doStep (src/agent_manager.cpp:29-50: the agent's next state is the
 * trajectory's state at time_step).  Control points are first truncated to float32 like TrajOptResult::desired_traj
 * (src/traj_optimizer.cpp:71-83); dim == 2: z := z_2d.  DEVICE pointers, asynchronous on `stream`.
 *   d_x [n][dim*M*(n+1)]   x_out of the solve        d_hdr [n]  (max_vel / max_acc are read from it)      d_sfc [n*M] or NULL
 *   d_valid_out [n]  1 = isSolValid would return true        d_state_out [n][9]  position, velocity, acceleration */
int lscqp_validate_step_device(lscqp_handle h, int64_t n, double time_step, double z_2d, const double* d_x,
                               const lscqp_header* d_hdr, const lscqp_box* d_sfc, int32_t* d_valid_out, double* d_state_out,
                               void* stream);

/* Safety metrics of one planned step, the figures MultiSyncSimulator::update accumulates for the reference's summary CSV
 * (src/multi_sync_simulator.cpp:486-577; log/summary_*.csv columns safety_ratio_agent, vel/acc excess): for each local
 * agent and each sample time s * record_time_step, s < n_samples (the reference samples while future_time <
 * multisim_time_step - 1e-5, :489), the smallest ellipsoidal distance to any other agent over the sum of the radii
 * (ellipsoidalDistance, include/util.hpp:155-159, radius-weighted downwash :505-507) and the positive parts of
 * (v_k - max_vel_k) / max_vel_k, (a_k - max_acc_k) / max_acc_k (:560-572).  States are Trajectory::getStateAt of the
 * float32 control points.  The mission-wide figures are the min / max of these per-agent records (over ranks: one
 * MIN / MAX all-reduce).  The obstacle safety ratio (:527-557) is lscqp_safety_obstacles_device below.
 *   d_x_all [n_total][dim*M*(n+1)]  every agent's current plan (x_out of the solve, all-gathered)
 *   d_radius, d_downwash [n_total]   d_hdr [n_agents] (max_vel / max_acc)   d_out [n_agents] */
typedef struct lscqp_safety {
    double safety_ratio;        /* min over samples and other agents; +inf if there is no other agent */
    int32_t closest_agent;      /* global id attaining it (first sample, then smallest id, like the reference's strict <) */
    int32_t sample;             /* sample index attaining it */
    double vel_excess_ratio[3]; /* max over samples, 0 where the limit is kept */
    double acc_excess_ratio[3];
} lscqp_safety;
int lscqp_safety_metrics_device(lscqp_handle h, int64_t n_agents, int64_t first_agent, int64_t n_total, int32_t n_samples,
                                double record_time_step, double z_2d, const double* d_x_all, const double* d_radius,
                                const double* d_downwash, const lscqp_header* d_hdr, lscqp_safety* d_out, void* stream);
/* The OBSTACLE leg of the same loop (src/multi_sync_simulator.cpp:527-557): per local agent the minimum, over the samples of its plan
 * and over the obstacles of the mission, of ellipsoidalDistance(agent position, obstacle position, downwash) / (r_i + r_o) with the
 * mixed downwash (r_o dw_o + r_i dw_i) / (r_i + r_o) (:538-540, include/util.hpp:155-159).  The obstacle table is the one the
 * constraint generator takes (lscqp_obstacle: position, radius, downwash are read); positions are the obstacle generator's CURRENT
 * ones, the same for every sample (:534 -- only the agents move along future_time), narrowed to float32 like point3d.  Entries with
 * type == LSCQP_OBSTACLE_REAL are skipped (:531-532: "real" obstacles are tracked robots, not simulated ones).  safety_ratio_obs is
 * +inf and closest_obstacle -1 when nothing was compared (SP_INFINITY in the reference).  MIN over ranks gives the mission's figure.
 *   d_x_all [n_total][dim*M*(n+1)], d_radius / d_downwash [n_total] (only the local agents' entries are read), d_obstacles [n_obstacles],
 *   d_out [n_agents] */
#define LSCQP_OBSTACLE_REAL 2
typedef struct lscqp_safety_obs {
    double safety_ratio_obs;  /* min over samples and obstacles */
    int32_t closest_obstacle; /* index into d_obstacles attaining it (first sample, then smallest index: the reference's strict <) */
    int32_t sample;
} lscqp_safety_obs;
int lscqp_safety_obstacles_device(lscqp_handle h, int64_t n_agents, int64_t first_agent, int64_t n_total, int32_t n_samples,
                                  double record_time_step, double z_2d, const double* d_x_all, const double* d_radius,
                                  const double* d_downwash, int32_t n_obstacles, const lscqp_obstacle* d_obstacles,
                                  lscqp_safety_obs* d_out, void* stream);

/* ---- next row of the path: the producer of the SFC boxes -----------------------------------
 *
 * A build-owned voxel map replaces the reference's octomap + DynamicEDTOctomap (both third-party, absent here):
 *   lscqp_map_create           MapManager::updateOctreeFromCSV (src/map_manager.cpp:262-305): the rows of the world CSV --
 *                              boxes [n_boxes][6] = centre x,y,z, size x,y,z -- are rasterised exactly as the reference
 *                              does, over the bounding box world_min .. world_max (DynamicEDTOctomap's, :13-14,74-76),
 *                              and every voxel gets its nearest occupied cell within max_dist (the reference passes 1.0 m):
 *                              exact Euclidean distance between cell centres.  Ties between equally near cells, which
 *                              dynamicEDT3D resolves by propagation order, go to the smallest (dz, dy), then the nearer
 *                              side with -x first.  HOST pointers; the map lives in HBM.
 *   lscqp_map_create_from_csv  the same from a world CSV file (the reference's CSVRange loop)
 *   lscqp_map_info / lscqp_map_download   grid size, first octomap key, and the two fields (for inspection and tests):
 *                              occ [dims[2]][dims[1]][dims[0]] bytes; nearest, same shape, int32:
 *                              (dx+128) | (dy+128)<<8 | (dz+128)<<16 | 1<<24, or 0 = none within max_dist
 * and the corridor of each agent is updated on the device, one workgroup (4 wavefronts) per agent:
 *   lscqp_construct_sfc_device, mode
 *     LSCQP_SFC_INIT        CollisionConstraints::initializeSFC (src/collision_constraints.cpp:366-384): all M boxes :=
 *                           expandSFC of the grid cell around the position; status 0 where the reference throws
 *     LSCQP_SFC_FROM_HULL   constructSFCFromConvexHull (:414-436; the default launch, goal mode grid_based_planner): boxes
 *                           shift down by one segment, the last one := expandSFCFromConvexHull of {last point, goal point,
 *                           next waypoint} (:692-722), else of {last point, goal point} inside the previous box (:724-775),
 *                           else the previous box (status 0)
 *     LSCQP_SFC_FROM_POINT  constructSFCFromPoint (:396-412): the last box := expandSFCFromPoint(last point) with the
 *                           goal-ordered axis candidates (setAxisCand :1134-1170), else the previous box (status 0)
 *   with isObstacleInSFC (:777-808), isSFCInBoundary (:810-817) and expandSFC (:819-946) in the reference's float32 /
 *   double arithmetic -- including its quirk: where the distance-map query finds no cell within max_dist (or the sample lies
 *   outside the map) `closest_point` stays default-constructed and the sample is measured against a cell at the WORLD ORIGIN
 *   (:796-800), which cuts corridors short within margin + res/2 of the origin.  (Round 1 treated that case as "no obstacle".)
 *   d_points [n][3][3]  per agent: position (INIT) or last point of the initial trajectory, current goal point, next waypoint
 *   d_radius [n]        Agent::radius (the margin)       d_sfc [n][M] boxes, updated in place       d_status_out [n] */
typedef struct lscqp_map_s* lscqp_map;
#define LSCQP_SFC_INIT 0
#define LSCQP_SFC_FROM_HULL 1
#define LSCQP_SFC_FROM_POINT 2
int lscqp_map_create(const double* boxes, int64_t n_boxes, const double* world_min, const double* world_max, double resolution,
                     double max_dist, lscqp_map* out);
int lscqp_map_create_from_csv(const char* path, const double* world_min, const double* world_max, double resolution,
                              double max_dist, lscqp_map* out);
void lscqp_map_destroy(lscqp_map map);
/* Optional acceleration of the corridor construction, once per map (set-up time: not concurrently with corridor launches on the map):
 * a summed-area table over the cells that could make an isObstacleInSFC test fail for an agent of radius <= max_radius.  A box of
 * sample points whose cell range holds none of them passes its test without a single point being evaluated -- in open space that
 * is every test of expandSFC, the whole-box re-tests included; all other boxes are evaluated exactly as without the table, so the
 * corridors are the same bit for bit.  4 bytes per map cell.  lscqp_plan_create calls it with the largest radius of its agents. */
int lscqp_map_prepare(lscqp_map map, double max_radius);
int lscqp_map_info(lscqp_map map, int32_t* dims, int32_t* key0);
int lscqp_map_download(lscqp_map map, uint8_t* occ, int32_t* nearest);
int lscqp_construct_sfc_device(lscqp_handle h, lscqp_map map, int32_t mode, int64_t n, const double* d_points,
                               const double* d_radius, lscqp_box* d_sfc, int32_t* d_status_out, void* stream);
/* The same with a work order (round 4): workgroup k of the launch builds the corridor of agent d_order[k] (a permutation of 0 .. n-1;
 * NULL = identity) and every agent's cost -- the cycles its workgroup took, >> 4 -- is left in d_cost_out[agent] (NULL: not recorded).
 * lscqp_order_by_cost_device sorts by the costs of the PREVIOUS replan, most expensive first (stable; 16 levels scaled to the largest):
 * a corridor along a wall costs three times one in open space and a launch ends with its last workgroup -- 4096 agents 0.98 -> 0.83 ms.
 * Same boxes bit for bit in any order; lscqp_plan carries costs and order from replan to replan by itself where its launches exceed the chip. */
int lscqp_order_by_cost_device(int64_t n, const uint32_t* d_cost_prev, int32_t* d_order_out, void* stream);
int lscqp_construct_sfc_device_ordered(lscqp_handle h, lscqp_map map, int32_t mode, int64_t n, const double* d_points,
                                       const double* d_radius, lscqp_box* d_sfc, int32_t* d_status_out, const int32_t* d_order,
                                       uint32_t* d_cost_out, void* stream);
/* Same, HOST pointers, synchronous; M boxes per agent (sfc is read and updated in place). */
int lscqp_construct_sfc(lscqp_map map, int32_t mode, int32_t M, int64_t n, const double* points, const double* radius,
                        lscqp_box* sfc, int32_t* status_out);

/* ---- the grid planner / MAPF layer (last row): each agent's next waypoint, on the device -------------------
 *
 * Device analogue of MultiSyncSimulator::decentralizedMAPP (reference src/multi_sync_simulator.cpp:160-303) in the default configuration
 * mode/goal = grid_based_planner, mode/mapf = pibt: the 0.5 m grid of GridBasedPlanner (src/grid_based_planner.cpp), one distance
 * table per agent (Solver::createDistanceTable, src/mapf/solver.cpp:270-289), ONE timestep of PIBT (src/mapf/pibt.cpp) per group of
 * agents in communication range, and the simulator's filter that decides which agents take their new waypoint.  2-D missions only.
 *   lscqp_grid_shape          GridBasedPlanner::updateGridInfo (:86-100): grid_min snaps the world box to multiples of the resolution
 *                             (SP_EPSILON = 1e-9), a 2-D mission has one plane at z_2d.  Host arithmetic only, no device call.
 *   lscqp_grid_create         the grid over the map's world box and updateGridMap (:102-140): a node is occupied when the L-infinity
 *                             distance to the nearest occupied voxel CELL is below radius - 1e-5, evaluated by a kernel from the map's
 *                             nearest-cell field with the corridor kernel's query -- a node without a cell within max_dist is measured
 *                             against a cell at the world origin, like lscqp_construct_sfc_device.  grid/margin is read by the reference
 *                             and used nowhere.  world_dimension != 2: LSCQP_ERR_UNSUPPORTED (the reference's MAPF graph is x-y only and
 *                             its 3-D waypoints come out at the floor of the world).
 *   lscqp_grid_info / _download   grid_min[3], dims[3]; the static occupancy, uint8 [dims[1]][dims[0]].  _download_mission: the occupancy
 *                             the last lscqp_grid_fields_device left (start and goal nodes cleared), which the waypoint decision reads.
 *   lscqp_grid_fields_device  updateGridMission (:255-283) + createDistanceTable for n agents: d_field [n][dims[1]][dims[0]] int32, the
 *                             number of 4-connected steps (left x-1, right x+1, up y-1, down y+1: Grid::Grid) from the node to the
 *                             agent's goal node, LSCQP_GRID_UNREACHABLE on occupied and unreachable nodes; d_init_d [n] = the field at
 *                             the agent's START node (PIBT's init_d).  One workgroup per agent relaxes its field in sweeps in LDS
 *                             (16 bits per node) up to 65 000 nodes, in HBM beyond.  d_start_points, d_goal_points [n][3].
 *     DIFFERENCE 1: the reference rebuilds every table in every replan and clears the current and goal nodes of the agents of ONE group
 *     at a time.  Goals and map do not change during a mission and a waypoint is always a free node except possibly the start, so here
 *     the start and goal nodes of EVERY agent passed in are cleared, once, and the fields are computed once per mission (lscqp_plan:
 *     per lscqp_plan_reset, and again when the map's generation counter moves).  The two rules differ only where a start or goal node
 *     lies inside an inflated cell AND the swarm is split into groups.  No replan then pays for n graph searches.
 *   lscqp_waypoints_device    one replan's decision for all n agents of the mission, asynchronous on `stream`:
 *       groups     connected components of "L-infinity distance of the current POSITIONS (d_state) < communication_range" (:162-193;
 *                  range < 0: one group; range == 0: every agent alone, and like range < 0 no range test in the filter; NaN is refused).  d_group_out [n]: the least agent id of the agent's group.
 *       PIBT       per group, first timestep (the simulator keeps path[1] only, :219-220; every `elapsed` is 0): priority init_d, then
 *                  tie_breaker = id / n, larger first; funcPIBT with priority inheritance and backtracking, chooseNode with vertex and
 *                  swap conflicts.  An agent's node is the node of its present WAYPOINT (:205).  Agents of other groups are invisible.
 *                  DIFFERENCE 2: std::shuffle in chooseNode is replaced by the identity order -- the candidates are visited as left,
 *                  right, up, down, stay and the first one wins a tie.  That is one of the orders the reference can draw, so every
 *                  result is one the reference could have produced.  d_desired_out [n]: the node taken, y * dims[0] + x.
 *       filter     (:222-296) a desired waypoint is taken only if (a) it lies within range / 2 - 1e-5 (L-infinity) of every segment start
 *                  point and of the last point of the agent's plan (d_plan [n][dim*M*6], the plans as the last replan left them; NULL:
 *                  of the agent's position -- no trajectory yet), (b) it differs from the present waypoint, (c) the agent's current goal
 *                  point (d_current_goal [n][3]) has reached the present waypoint, (d) no member of its group that keeps its waypoint
 *                  holds that node.  d_waypoint [n][3] is updated in place, d_updated_out [n] = 1 where it changed.
 *                  DIFFERENCE 3: the reference drops repeated leading configurations of the PIBT plan (:355-374) and treats an empty
 *                  plan as "MAPF failed"; with one timestep neither exists: a replan in which nobody can move leaves every waypoint.
 *     Precondition (PIBT's own): the agents of one group hold distinct waypoint nodes.  Where two do, the one with the larger id is the
 *     node's holder, as in PIBT::run.  An agent's own node counts as free for it whatever the map says.
 *     The decision loop has a hard bound of 4 n + 16 passes (funcPIBT is entered at most once per agent: 3 n suffice); reaching it
 *     leaves every waypoint as it was and sets the status word lscqp_grid_status reads (0 = fine, 1 = bound reached).  The word is sticky:
 *     later decisions do not clear it; lscqp_grid_fields_device (hence lscqp_plan_reset) does.  The grid keeps nothing of the map after
 *     lscqp_grid_create: it may outlive it.
 *     The launch uses work arrays owned by the grid: one decision at a time per grid.  They grow on demand, which synchronises and
 *     allocates -- a caller that captures the launch in a graph calls lscqp_grid_reserve(grid, n) first.
 *   lscqp_waypoints_wide_device   the SAME decision -- same arguments, same contract, same status word, every output equal to
 *     lscqp_waypoints_device's bit for bit -- spread over the device for a large swarm instead of run by one workgroup.  After the same
 *     gather: groups from a cell list over the positions (a counting sort by x-y cell of side >= 1.0001 * range, enlarged until at most
 *     2 n + 16 cells cover the grid's box; positions outside fall into the edge cells) and a lock-free union-find over the pairs of the
 *     3 x 3 cells that pass the unchanged test, the root with the larger id hooked under the smaller -- O(n) work where agents are spread
 *     out, against n^2 per round; agents alone in their group decide in parallel; the others are sorted group by group (init_d
 *     descending, id descending) and ONE workgroup per group of more than one agent runs the PIBT walk by one of its wavefronts over
 *     node tables of the group's own (open-addressed, 4 n_g to 8 n_g slots: O(n) memory in all), with a bound of 4 n_g + 16 passes of its
 *     own, then the update filter for its members.  A last launch applies the updates; if ANY group reached its bound no waypoint of the
 *     swarm changes and the status word becomes 1.  Asynchronous on `stream`: 6 launches (range <= 0) or 11, none of which waits for
 *     another workgroup, no host round trip, capturable.  The walk inside one group stays sequential: a swarm that is one group
 *     (range < 0) gains from the sort only.  Work arrays: lscqp_grid_reserve_wide(grid, n), which includes lscqp_grid_reserve(grid, n)
 *     and adds about 150 bytes per agent; like the one-workgroup entry the wide entry allocates on demand (and synchronises) when nothing
 *     was reserved.  lscqp_grid_reserve and lscqp_waypoints_device keep their footprint.  One decision at a time per grid, either form. */
typedef struct lscqp_grid_s* lscqp_grid;
typedef struct lscqp_grid_desc {
    double resolution;       /* grid/resolution, 0.5 m in the launch files */
    double radius;           /* agent_radius of updateGridMap (the reference passes mission.agents[0].radius) */
    double z_2d;             /* world_z_2d */
    int32_t world_dimension; /* 2 */
    int32_t reserved_;
} lscqp_grid_desc;
#define LSCQP_GRID_UNREACHABLE 0x3fffffff /* larger than any path */
int lscqp_grid_shape(const double* world_min, const double* world_max, double resolution, int32_t world_dimension, double z_2d,
                     double* grid_min, int32_t* dims);
int lscqp_grid_create(lscqp_map map, const lscqp_grid_desc* desc, lscqp_grid* out);
void lscqp_grid_destroy(lscqp_grid grid);
int lscqp_grid_info(lscqp_grid grid, double* grid_min, int32_t* dims);
int lscqp_grid_download(lscqp_grid grid, uint8_t* occ);
int lscqp_grid_download_mission(lscqp_grid grid, uint8_t* occ);
int lscqp_grid_reserve(lscqp_grid grid, int64_t n);
int lscqp_grid_status(lscqp_grid grid, int32_t* status_out); /* waits for the device */
int lscqp_grid_fields_device(lscqp_grid grid, int64_t n, const double* d_start_points, const double* d_goal_points, int32_t* d_field,
                             int32_t* d_init_d, void* stream);
int lscqp_waypoints_device(lscqp_grid grid, double communication_range, int32_t M, int32_t dim, int64_t n, const double* d_state,
                           const double* d_plan, const double* d_current_goal, const int32_t* d_field, const int32_t* d_init_d,
                           double* d_waypoint, int32_t* d_group_out, int32_t* d_desired_out, int32_t* d_updated_out, void* stream);
int lscqp_grid_reserve_wide(lscqp_grid grid, int64_t n);
int lscqp_waypoints_wide_device(lscqp_grid grid, double communication_range, int32_t M, int32_t dim, int64_t n, const double* d_state,
                                const double* d_plan, const double* d_current_goal, const int32_t* d_field, const int32_t* d_init_d,
                                double* d_waypoint, int32_t* d_group_out, int32_t* d_desired_out, int32_t* d_updated_out, void* stream);

/* ---- the caller of the path: one replan of a batch of agents as one chain of device work ----------
 *
 * Device analogue of TrajPlanner::plan / planImpl (reference src/traj_planner.cpp:33-60, 117-139) run for every local agent of
 * the mission at once, and of the loop around it in MultiSyncSimulator (src/multi_sync_simulator.cpp:305-400).  A plan object
 * owns the state the reference's planners carry from replan to replan -- previous plans (TrajPlanner::prev_traj), current goal
 * points, corridors -- plus the work buffers, all in HBM, and enqueues
 *     obstaclePrediction / initialTrajPlanning (:228-319, 360-423; all three modes,    lscqp_shift_traj(_partial)_device + the chain's
 *       checkObstacleDisturbance)                                                       prepare step
 *     broadcastMsgs' range filter (src/multi_sync_simulator.cpp:318-333)              lscqp_select_neighbours_device
 *     constructLSC (:552-569)                                                         lscqp_generate_constraints_device
 *     constructSFC / generateSFC (:571-579, 738-753; initializeSFC on the first replan) lscqp_construct_sfc_device
 *     goalPlanningWithGridBasedPlanner (:545-550)                                     lscqp_optimize_goal_device; the goal is then
 *                                                                                     held as point3d (float32) and
 *                                                                                     getTerminalSegments_old is evaluated with
 *                                                                                     octomap's float32 arithmetic
 *     trajOptimization (:755-803)                                                     lscqp_solve_batch_device_ex with the initial
 *                                                                                     trajectory as the start and the device-side
 *                                                                                     second pass; a QP that is not OPTIMAL leaves
 *                                                                                     desired_traj = initial_traj (failsafe :796-797)
 *     prev_traj = desired_traj (:51); AgentManager::doStep (src/agent_manager.cpp:29-50)  plans updated in place;
 *                                                                                     lscqp_validate_step_device (isSolValid is
 *                                                                                     reported, not acted on: the reference consults
 *                                                                                     it in DLSC mode only, :763-766)
 * on ONE stream, with no host synchronisation, allocation or copy in between.  lscqp_plan_step_graph captures that chain once in
 * a hipGraph and replays it: one graph launch per replan instead of ten kernel launches.
 * Where the waypoints come from is the plan's waypoint_mode: LSCQP_WAYPOINT_FROM_CALLER -- the caller's grid planner / MAPF layer writes each
 * local agent's next waypoint into LSCQP_PLAN_BUF_WAYPOINT before the step -- or LSCQP_WAYPOINT_GRID_PIBT: the chain starts with
 * lscqp_waypoints_device (decentralizedMAPP precedes the planning loop in the simulator too) and a mission flies from start points and
 * goal points alone: lscqp_plan_reset, then lscqp_plan_step_graph in a loop, with no host work between replans.  (Unless closed_loop is
 * set, the simulator writes the agents' states.)
 * Dynamic (non-agent) obstacles join the chain through lscqp_plan_set_obstacles ("dynamic obstacles in the chain" below): they move on
 * the device from replan to replan, take the first row slots of every agent and enter the safety figures.  A plan without them
 * enqueues the chain described here, node for node.
 * Sharding (section 8e): rank r owns the agents [first_agent, first_agent + n_agents) of n_total; its plan needs every agent's
 * previous plan, state and goal point, so the owners' slices of LSCQP_PLAN_BUF_PLAN / _STATE / _GOAL are all-gathered between
 * steps (lscqp_allgather; the layout is [n_total][...] on every rank, so the gather is in place). */
typedef struct lscqp_plan_s* lscqp_plan;
typedef struct lscqp_agent_param { /* the Agent fields the chain reads (include/sp_const.hpp Agent; mission file values) */
    double radius, downwash;
    double max_vel[3], max_acc[3];
    double nominal_velocity;
} lscqp_agent_param;
typedef struct lscqp_plan_desc {
    int64_t n_agents;        /* local agents */
    int64_t n_total;         /* agents of the mission (each other's obstacles) */
    int64_t first_agent;     /* global id of local agent 0 */
    int32_t n_obs;           /* row slots per agent: in-range agents beyond it are cut to the nearest ones and reported in
                                LSCQP_PLAN_BUF_IN_RANGE (> n_obs), never silently */
    int32_t constraint_mode; /* LSCQP_GEN_LSC / _CLSC / _BVC (constructLSC's switch, :555-566) */
    int32_t sfc_mode;        /* LSCQP_SFC_FROM_HULL (goal mode grid_based_planner) or LSCQP_SFC_FROM_POINT; ignored without a map */
    int32_t optimize_goal;   /* != 0: GoalOptimizer moves the goal point towards the waypoint (goal mode grid_based_planner);
                                0: the goal points are left as the caller set them (static goal modes) */
    int32_t closed_loop;     /* != 0: the local agents' next states (doStep) become their current states for the next replan */
    int32_t safety_samples;  /* > 0: the step ends with the safety figures of MultiSyncSimulator::update over this many samples of the
                                new plans (lscqp_safety_metrics_device; needs n_agents == n_total: every agent's new plan), 0: off */
    double time_step;        /* multisim_time_step: == dt shifts the plans by one segment, < dt uses Segment::subSegment */
    double z_2d;             /* world_z_2d of 2-D missions */
    double record_time_step; /* spacing of the safety samples (multisim_save_time_step) */
    int32_t tight_warm_start; /* != 0: the plan's QP solves centre their warm starts in LSCQP_WARM_TIGHT mode whatever the handle's class
                                 says (a private clone of the class).  Pays where the plans barely change from replan to replan (agents
                                 holding position: forest10 chain 413 -> 320 us); with agents on the move it does not (10 agents: equal,
                                 64 / 256 agents: 20 % slower, the batch waits for its slowest QP) -- hence off by default */
    int32_t prediction_mode;  /* how the OTHER agents' trajectories are predicted (obstaclePrediction, src/traj_planner.cpp:228-253):
                                 LSCQP_TRAJ_FROM_PREVIOUS_SOLUTION (0; mode/planner lsc and dlsc, src/param.cpp:127-166: their shifted
                                 previous plans; constant velocity on the first replan, :276-279), _FROM_POSITION (mode/planner bvc:
                                 they stay where they are) or _FROM_VELOCITY (circle_test: Trajectory::planConstVelTraj from the
                                 current state) */
    int32_t initial_traj_mode; /* the planning agent's own initial trajectory (initialTrajPlanning, :360-423): same three values */
    int32_t waypoint_mode;     /* LSCQP_WAYPOINT_FROM_CALLER (0): LSCQP_PLAN_BUF_WAYPOINT is the caller's to write.  LSCQP_WAYPOINT_GRID_PIBT (1):
                                  the plan owns a lscqp_grid over its map (resolution 0.5 m, lscqp_plan_set_grid changes it; radius of agent 0,
                                  as the reference passes it) and every replan starts with lscqp_waypoints_device over the plans, states and
                                  goal points the last replan left.  Needs a map, a 2-D class and every agent's waypoint and plan on this
                                  device: n_agents == n_total (LSCQP_ERR_INVALID_ARGUMENT otherwise, the rule of safety_samples) */
    double reset_threshold;   /* checkObstacleDisturbance (:312-319, plan/reset_threshold, 0.1 in the launch files): an agent whose predicted
                                 trajectory starts further than this from its current position is predicted to stay where it is
                                 (a disturbed or externally moved robot; only with closed_loop == 0 can that happen).  <= 0: no check */
} lscqp_plan_desc;
#define LSCQP_TRAJ_FROM_PREVIOUS_SOLUTION 0
#define LSCQP_TRAJ_FROM_POSITION 1
#define LSCQP_TRAJ_FROM_VELOCITY 2
#define LSCQP_WAYPOINT_FROM_CALLER 0
#define LSCQP_WAYPOINT_GRID_PIBT 1
/* Buffers of a plan (device pointers through lscqp_plan_buffer; lscqp_plan_upload / _download copy synchronously).
 * "all": [n_total] entries indexed by global id; "local": [n_agents] entries. */
#define LSCQP_PLAN_BUF_STATE 0        /* in   all    double[9]: position, velocity, acceleration (float32 values, as State holds them) */
#define LSCQP_PLAN_BUF_WAYPOINT 1     /* in   local  double[3]: agent.next_waypoint */
#define LSCQP_PLAN_BUF_PLAN 2         /* i/o  all    double[dim*M*6]: previous plans in, the local agents' new plans out */
#define LSCQP_PLAN_BUF_GOAL 3         /* i/o  all    double[3]: current goal points; the local agents' are updated */
#define LSCQP_PLAN_BUF_HEADER 4       /* out  local  lscqp_header of the last replan */
#define LSCQP_PLAN_BUF_ROWS 5         /* out  local  lscqp_row[n_obs*M*6] of the last replan */
#define LSCQP_PLAN_BUF_SFC 6          /* i/o  local  lscqp_box[M]: corridors */
#define LSCQP_PLAN_BUF_STATUS 7       /* out  local  int32: LSCQP_STATUS_* of the QP */
#define LSCQP_PLAN_BUF_GOAL_STATUS 8  /* out  local  int32: LSCQP_STATUS_* of the goal LP */
#define LSCQP_PLAN_BUF_SFC_STATUS 9   /* out  local  int32: 1 = corridor updated, 0 = previous box kept / seed inside an obstacle */
#define LSCQP_PLAN_BUF_VALID 10       /* out  local  int32: isSolValid */
#define LSCQP_PLAN_BUF_IN_RANGE 11    /* out  local  int32: agents within communication range */
#define LSCQP_PLAN_BUF_NEXT_STATE 12  /* out  local  double[9]: state at time_step along the new plan (closed_loop: the local slice of
                                         LSCQP_PLAN_BUF_STATE itself) */
#define LSCQP_PLAN_BUF_OBJECTIVE 13   /* out  local  double */
#define LSCQP_PLAN_BUF_INFO 14        /* out  local  lscqp_info */
#define LSCQP_PLAN_BUF_SAFETY 15      /* out  local  lscqp_safety (safety_samples > 0) */
/* waypoint_mode = LSCQP_WAYPOINT_GRID_PIBT only (no such buffer otherwise: lscqp_plan_buffer returns NULL and 0 bytes) */
#define LSCQP_PLAN_BUF_DESIRED_GOAL 16     /* in   all    double[3]: the mission's goal points (Agent::desired_goal_point), set by lscqp_plan_reset */
#define LSCQP_PLAN_BUF_WAYPOINT_UPDATED 17 /* out  local  int32: 1 = the last replan moved the agent's waypoint */
#define LSCQP_PLAN_BUF_GROUP 18            /* out  local  int32: least agent id of the agent's communication group in the last replan */
#define LSCQP_PLAN_BUF_COUNT 19
/* agents [n_total] (host).  map: required exactly when the class uses corridors.  The class's row_format must be LSCQP_ROWS_F64. */
int lscqp_plan_create(lscqp_handle h, lscqp_map map, const lscqp_plan_desc* desc, const lscqp_agent_param* agents, lscqp_plan* out);
void lscqp_plan_destroy(lscqp_plan plan);
/* Mission start (host pointers, synchronous): every agent hovers at its start position [n_total][3] (the plans the reference's
 * planners start from, planner_seq < 2), goal points := goal_points, or the start positions if NULL (AgentManager's constructor),
 * waypoints := the goal points; the next step is a FIRST replan (initializeSFC). */
int lscqp_plan_reset(lscqp_plan plan, const double* start_positions, const double* goal_points);
/* waypoint_mode = LSCQP_WAYPOINT_GRID_PIBT: goal_points are the mission's DESIRED goal points (required); the current goal points and the
 * waypoints := the start positions (AgentManager's constructor, src/agent_manager.cpp:8-10) and the distance fields of the mission are
 * computed (lscqp_grid_fields_device).  lscqp_plan_set_grid replaces the plan's grid by one of another resolution; call it before
 * lscqp_plan_reset.  lscqp_plan_grid: the plan's grid (NULL in mode 0), for lscqp_grid_info / _download / _status. */
int lscqp_plan_set_grid(lscqp_plan plan, double resolution);
lscqp_grid lscqp_plan_grid(lscqp_plan plan);
void* lscqp_plan_buffer(lscqp_plan plan, int32_t which, uint64_t* bytes_out);
int lscqp_plan_upload(lscqp_plan plan, int32_t which, const void* host, uint64_t offset, uint64_t bytes);
int lscqp_plan_download(lscqp_plan plan, int32_t which, void* host, uint64_t offset, uint64_t bytes);
/* One replan of all local agents, asynchronous on `stream` (hipStream_t as void*; NULL = default stream). */
int lscqp_plan_step(lscqp_plan plan, void* stream);
/* The same through a hipGraph captured at the first call that is not a first replan (that one runs eagerly: it differs, and it
 * warms the kernels' one-time attributes up).  Results are bit-for-bit those of lscqp_plan_step.  The captured launches carry the
 * solver class by value; the plan notices lscqp_update(h) / lscqp_map_prepare(map) by their generation counters, drops the graph and
 * re-captures at the next call (both step entry points).  An update that changes the SHAPE the plan was sized for -- segments,
 * dimension, corridor rows on/off, row format, a neighbour capacity below desc.n_obs, dt below desc.time_step -- is refused with
 * LSCQP_ERR_INVALID_ARGUMENT at the next step: such a plan has to be destroyed and created again. */
int lscqp_plan_step_graph(lscqp_plan plan, void* stream);
int64_t lscqp_plan_graph_nodes(lscqp_plan plan); /* nodes of the captured graph, 0 before the capture */
/* One replan of a mission spread over the devices of a communicator (section 8e): plans[g] was created with device g of `c` current
 * (its own handle and map live there too) and owns the block [first_agent, first_agent + n_agents) of the n_total agents, blocks
 * consecutive in device order and covering the mission.  Every plan's chain is enqueued on its device's stream
 * (lscqp_comm_stream), eagerly or through its graph, followed on the same streams by the one exchange the reference has --
 * MultiSyncSimulator::broadcastMsgs, src/multi_sync_simulator.cpp:305-352: every planner receives the others' previous plans --
 * as an in-place RCCL exchange of the owners' slices of LSCQP_PLAN_BUF_PLAN / _STATE / _GOAL (grouped ncclAllGather for equal
 * blocks, one ncclBroadcast per owner otherwise).  Asynchronous: lscqp_comm_synchronize waits for all devices.  Waypoints are
 * written per plan before the call, as for lscqp_plan_step. */
int lscqp_plan_group_step(lscqp_comm c, const lscqp_plan* plans, int32_t use_graph);

/* ---- many missions over one map: a mission partition of a plan's agents --------------------------------------------------------------
 *
 * The reference is evaluated on sets of missions (launch/test_all_*.launch: missions/<set>/<set>_1..30.json, one result line per
 * mission), mission k over world k of a set of worlds of one shape -- see "each mission over its own world" below for the worlds; with
 * ONE map every mission of the plan flies over that map.  A partition lets one plan fly K such missions in one chain per replan.  Missions are contiguous ranges of global
 * agent ids, [mission_offsets[k], mission_offsets[k + 1]), the list strictly increasing from 0 to n_total (no empty mission).  Agents of
 * different missions share the map and the solver class and nothing else: they are never each other's neighbours (no LSC / BVC rows for
 * each other), never in one communication group, never compete for a grid node, never enter each other's safety figures, and their start
 * and goal nodes are cleared in their own mission's occupancy only.  Everything else in the chain is per agent and unchanged.
 *   lscqp_plan_set_missions   host offsets [n_missions + 1].  Call it before lscqp_plan_reset, like lscqp_plan_set_grid: it waits for the
 *                             device, drops a captured graph and invalidates the distance fields, and a step before the next
 *                             lscqp_plan_reset is refused (LSCQP_ERR_INVALID_ARGUMENT).  n_missions <= 1 or NULL offsets: back to the single
 *                             mission, whose chain is the one a plan without this call runs, launch for launch.  A bad offset list and a
 *                             sharded plan (n_agents != n_total, the rule of safety_samples and waypoint_mode 1) are refused and leave the
 *                             plan as it was.  Out of scope: different classes or n_obs per mission; missions across devices (a map per mission:
 *                             lscqp_plan_set_worlds, which refuses another mission count here while worlds are set).
 *   lscqp_plan_missions       the partition read back: *n_missions_out (1 without a partition) and, if offsets_out != NULL, its
 *                             n_missions + 1 offsets.
 *   lscqp_plan_mission_status status_out [n_missions], host; waits for the device.  The word of each mission's waypoint walk: 0 = fine,
 *                             1 = the bound of 4 n_k + 16 passes was reached (n_k: the mission's agents), which leaves the waypoints of THAT
 *                             mission alone.  Sticky like lscqp_grid_status, cleared by lscqp_plan_reset; all zero in waypoint_mode 0.
 *                             LSCQP_PLAN_BUF_GROUP keeps reporting the least GLOBAL id of the agent's group.
 * The mission-aware twins of the entry points in which agents see each other.  Each takes the partition twice: mission_offsets on the
 * host (checked before the device is touched; the safety launch is shaped by the largest mission) and d_mission_offsets, the same
 * n_missions + 1 values on the device, which the kernels read.  All n agents are local (no first_agent); ids in and out are global.
 *   lscqp_select_neighbours_missions_device   lscqp_select_neighbours_device with the agent's own mission as its candidates; the cut to the
 *                             n_obs nearest and the in-range count keep their meaning.
 *   lscqp_safety_metrics_missions_device      lscqp_safety_metrics_device over the pairs within a mission; closest_agent is a global id,
 *                             -1 and an infinite ratio for a mission of one.
 *   lscqp_grid_fields_missions_device         lscqp_grid_fields_device with one occupancy copy per mission: an agent's start and goal nodes
 *                             are cleared in its mission's copy, and its field is relaxed over that copy.  Clears the status words.
 *   lscqp_waypoints_missions_device           lscqp_waypoints_device as one workgroup per mission over its slice: groups, priorities, the
 *                             PIBT walk with node tables of its own (LDS up to 60 KB, a slab of an HBM buffer per mission beyond) and the
 *                             filter.  d_group_out: least global id of the group.  lscqp_grid_fields_missions_device over the SAME
 *                             partition must have come last on this grid (it makes the copies and clears them for the agents of its
 *                             partition): any other offset list is refused.  One decision at a time per grid.
 *   lscqp_grid_mission_status status_out [n_missions], host; waits: the words lscqp_plan_mission_status reports.
 * Which form of the waypoint decision a plan's chain starts with (waypoint_mode = LSCQP_WAYPOINT_GRID_PIBT only; any other plan:
 * LSCQP_ERR_INVALID_ARGUMENT):
 *   lscqp_plan_set_waypoint_decision   LSCQP_DECISION_ONE_WORKGROUP (the default: lscqp_waypoints_device, the chain node for node as it
 *                             was), LSCQP_DECISION_WIDE (lscqp_waypoints_wide_device) or LSCQP_DECISION_AUTO (wide from
 *                             LSCQP_DECISION_AUTO_MIN_AGENTS agents of the mission on; NOTES.md section 20 says where that figure comes from).  Every buffer of
 *                             the plan is bit-identical whichever is chosen.  The call waits for the device, reserves the work arrays
 *                             (lscqp_grid_reserve_wide) and drops a captured graph, like lscqp_plan_set_missions; no lscqp_plan_reset
 *                             is needed after it.  A partition of more than one mission keeps one workgroup per mission: WIDE or AUTO on
 *                             a plan that has one, and such a partition on a plan set to WIDE or AUTO, are LSCQP_ERR_UNSUPPORTED and
 *                             leave the plan as it was. */
#define LSCQP_DECISION_ONE_WORKGROUP 0
#define LSCQP_DECISION_WIDE 1
#define LSCQP_DECISION_AUTO 2
#define LSCQP_DECISION_AUTO_MIN_AGENTS 512
int lscqp_plan_set_waypoint_decision(lscqp_plan plan, int32_t which);
int lscqp_plan_set_missions(lscqp_plan plan, int32_t n_missions, const int64_t* mission_offsets);
int lscqp_plan_missions(lscqp_plan plan, int32_t* n_missions_out, int64_t* offsets_out);
int lscqp_plan_mission_status(lscqp_plan plan, int32_t* status_out);
int lscqp_select_neighbours_missions_device(lscqp_handle h, int64_t n_total, int32_t n_missions, const int64_t* mission_offsets,
                                            const int64_t* d_mission_offsets, int32_t n_obs, double communication_range,
                                            const double* d_positions, int32_t* d_neighbours_out, int32_t* d_count_out, void* stream);
int lscqp_safety_metrics_missions_device(lscqp_handle h, int64_t n_total, int32_t n_missions, const int64_t* mission_offsets,
                                         const int64_t* d_mission_offsets, int32_t n_samples, double record_time_step, double z_2d,
                                         const double* d_x_all, const double* d_radius, const double* d_downwash, const lscqp_header* d_hdr,
                                         lscqp_safety* d_out, void* stream);
int lscqp_grid_fields_missions_device(lscqp_grid grid, int64_t n, int32_t n_missions, const int64_t* mission_offsets,
                                      const int64_t* d_mission_offsets, const double* d_start_points, const double* d_goal_points,
                                      int32_t* d_field, int32_t* d_init_d, void* stream);
int lscqp_waypoints_missions_device(lscqp_grid grid, double communication_range, int32_t M, int32_t dim, int64_t n, int32_t n_missions,
                                    const int64_t* mission_offsets, const int64_t* d_mission_offsets, const double* d_state,
                                    const double* d_plan, const double* d_current_goal, const int32_t* d_field, const int32_t* d_init_d,
                                    double* d_waypoint, int32_t* d_group_out, int32_t* d_desired_out, int32_t* d_updated_out, void* stream);
int lscqp_grid_mission_status(lscqp_grid grid, int32_t n_missions, int32_t* status_out);

/* ---- each mission over its own world: a set of maps of one shape ------------------------------------------------------------------------
 *
 * The reference's evaluation sets pair mission k with world k (launch/test_all_forest.launch names a mission directory and a world
 * directory of thirty files each; Mission::loadMission, src/mission.cpp:82-92, pairs them by index when the lists are equally long, and
 * multi_sync_simulator_node.cpp:44-59 loops over the pairs): thirty missions over thirty worlds of ONE SHAPE -- same world box, same
 * resolution, different pillars.  Two steps of a replan read the map: the corridor kernel and the grid's static occupancy.
 *   lscqp_worlds_create      n_worlds >= 1 maps on the current device that agree in resolution, world box (as float32), key0, dims and
 *                            max_dist; anything else is LSCQP_ERR_INVALID_ARGUMENT naming the first differing member and field.  The set
 *                            BORROWS its maps (they must outlive it; one map may appear twice) and owns one small device table: per world
 *                            the address of the nearest-cell field and of the free-space table.
 *   lscqp_worlds_prepare     lscqp_map_prepare on every member with one margin -- max_radius, or the largest margin a member already has a
 *                            table for -- and the table rewritten.  The corridor kernel carries the margin by value, so one margin serves
 *                            all worlds: if a member has no table, or the members' margins differ (one was prepared directly), a launch
 *                            uses no table at all -- every test is evaluated, the boxes are the same bit for bit.
 *   lscqp_worlds_info        *n_worlds, and dims[3] / key0[3] of the common shape (either may be NULL).
 *                            The set's own work (its table, lscqp_worlds_prepare, lscqp_worlds_destroy) and lscqp_grid_set_worlds run on
 *                            the device the set / the grid lives on, whichever is current; a LAUNCH with another device current is refused.
 *   lscqp_construct_sfc_worlds_device   lscqp_construct_sfc_device_ordered in which agent a is tested against world d_world_of[a]
 *                            (int32 [n], device).  The index belongs to the AGENT: with a work order, workgroup k builds agent d_order[k]
 *                            in world d_world_of[d_order[k]].  PRECONDITION: every index lies in [0, n_worlds); the kernel does not test
 *                            it.  A member prepared behind the set's back is noticed through its generation counter: the table is
 *                            rewritten before the launch (which waits for the device), or -- on a stream that is being captured -- the
 *                            launch is refused.  A stale address is never launched.  The kernel fetches its agent's two addresses once,
 *                            two scalar loads per workgroup, and then runs the statements of lscqp_construct_sfc_device.
 *   lscqp_grid_set_worlds    the grid's base occupancy per world: updateGridMap once per member into [n_worlds][nodes], with the
 *                            arithmetic of lscqp_grid_create.  The worlds' box must give the grid's own shape.  The grid keeps nothing of
 *                            the maps.  lscqp_grid_fields_missions_device then starts mission k's copy from base k and refuses a partition
 *                            whose n_missions differs from the world count; the one-mission entries (lscqp_grid_fields_device,
 *                            lscqp_waypoints_device, lscqp_waypoints_wide_device) refuse such a grid with LSCQP_ERR_UNSUPPORTED.
 *                            NULL: back to the one base of lscqp_grid_create.  lscqp_grid_download_world: base k, uint8 [dims[1]][dims[0]].
 *   lscqp_plan_set_worlds    world k for mission k of the plan's partition.  Like lscqp_plan_set_missions it waits for the device, drops a
 *                            captured graph and invalidates the distance fields, and a step before the next lscqp_plan_reset is refused.
 *                            Refused, the plan left as it was: no partition or one whose mission count differs from the world count; a
 *                            shape or device other than that of the map the plan was created with; a class without corridors.  While
 *                            worlds are set lscqp_plan_set_missions with another count is refused; one with the same count and other
 *                            offsets is taken, and the agents' world index follows it: an agent that changes mission changes world.  The plan's corridor node becomes the
 *                            worlds launch (work order and cost carry-over as before), in waypoint_mode 1 its grid gets the worlds
 *                            (lscqp_plan_set_grid re-applies them), the members are prepared through lscqp_worlds_prepare with the agents'
 *                            largest radius -- the last step of the call that can fail and the one that reaches beyond the plan: where it
 *                            has to rebuild a member's free-space table that map's generation counter moves, and every OTHER plan over
 *                            that map drops its captured graph (and re-makes its grid) at its next step, also when this call is refused
 *                            behind it --, and the generation check in front of every step covers every member.  The set must outlive
 *                            the plan or be taken away first.  NULL: back to the one map -- such a plan, and one that never saw the call,
 *                            enqueues the chain it always did node for node.  Dynamic obstacles given by lscqp_plan_set_obstacles are
 *                            shared by all missions, those of lscqp_plan_set_mission_obstacles are each mission's own; the record and
 *                            lscqp_plan_run do not know.  Out of scope: worlds of different shape; sharded plans; 3-D grids. */
typedef struct lscqp_worlds_s* lscqp_worlds;
int lscqp_worlds_create(const lscqp_map* maps, int32_t n_worlds, lscqp_worlds* out);
void lscqp_worlds_destroy(lscqp_worlds worlds);
int lscqp_worlds_prepare(lscqp_worlds worlds, double max_radius);
int lscqp_worlds_info(lscqp_worlds worlds, int32_t* n_worlds, int32_t* dims, int32_t* key0);
int lscqp_construct_sfc_worlds_device(lscqp_handle h, lscqp_worlds worlds, int32_t mode, int64_t n, const int32_t* d_world_of,
                                      const double* d_points, const double* d_radius, lscqp_box* d_sfc, int32_t* d_status_out,
                                      const int32_t* d_order, uint32_t* d_cost_out, void* stream);
int lscqp_grid_set_worlds(lscqp_grid grid, lscqp_worlds worlds);
int lscqp_grid_download_world(lscqp_grid grid, int32_t k, uint8_t* occ);
int lscqp_plan_set_worlds(lscqp_plan plan, lscqp_worlds worlds);

/* ---- the mission record: each mission's summary figures kept on the device, and plans flown to the finish -----------------------------
 *
 * What the reference prints per mission is its summary line (MultiSyncSimulator::saveSummarizedResultAsCSV, src/multi_sync_simulator.cpp
 * :658-709): flight time, flight distance, safety ratio, excess ratios.  A record keeps the running figures of that line per mission of a
 * partition (or for the whole swarm), accumulated by ONE kernel at the end of each replan (csrc/lscrecord.hip: one workgroup per mission),
 * and tells when a mission is over -- MultiSyncSimulator::isFinished (:401-424).  The host reads it when it likes.
 * The replan index r of a mission counts from 0 at the reset and lives in the record on the device (`replans` is the next r): a captured
 * graph carries constant arguments, so a host counter could not reach the kernel.  At the end of replan r, for every mission not finished:
 *   1. replan r is accumulated.
 *      - sample points: for every agent the n_samples points of its NEW plan at s * record_time_step -- the states the safety kernel
 *        evaluates (Trajectory::getStateAt of the float32 control points, z := z_2d in 2-D; the same device function), written to the points
 *        buffer.
 *      - distance (getTotalDistance, :711-720): the agent's distance grows by the norm() of consecutive points, the segment from the previous
 *        replan's last point to this replan's sample 0 included (none at r = 0), in octomath::Vector3's arithmetic: float differences, float
 *        sum of squares (no fused multiply-add), sqrt of that value in double; the sum is a double per agent.  The mission's distance is the
 *        sum of its agents' distances in id order, formed on the host at the download: a fixed order, bit-reproducible.
 *      - safety and excess ratios from the replan's lscqp_safety records: the mission's minimum safety_ratio with the replan, agent and other
 *        agent attaining it (strict < in the order replan, then agent id), per-axis maxima of the excess ratios (never below 0).
 *      - counts: agent-replans with a QP status != LSCQP_STATUS_OPTIMAL and the first replan with one (-1: none; the reference's loop ends at
 *        the first QPFAILED, here the flight goes on and the record names the replan), valid == 0, goal LP status != 0, sfc_status == 0,
 *        waypoint updates (where that buffer exists), the largest in-range count, agent-replans with in_range > the header's n_obs.
 *   2. the finish test, on the state replan r STARTED from (p0 of the headers): the mission has finished when no agent has
 *      distance(p0, desired goal) > goal_threshold -- Vector3::distance on float32 values (the goal narrowed to float32), compared in double;
 *      equality counts as finished.  Then finished = 1, replans = r + 1, flight_time = r * time_step: isFinished runs before doStep in the
 *      reference's loop, so the replan that starts from a passing state has been flown and logged.  A finished mission's record is frozen
 *      (its workgroup returns after loading one word; its agents go on being replanned: they hover) and never un-finishes.
 * lscqp_record_create      n_missions / offsets as lscqp_plan_set_missions takes them (HOST offsets; NULL: one mission [0, n_total)); M, dim
 *                          and dt are the class's.  time_step: the simulation step a replan stands for (flight_time's unit).
 * lscqp_record_reset       host goal points [n_total][3] (narrowed to float32 as they are); clears every figure; synchronous.
 * lscqp_record_step_device one accumulation, asynchronous on `stream`; DEVICE pointers indexed by global agent id: d_hdr [n_total], d_x_all
 *                          [n_total][dim*M*6], the int32 status buffers of the chain, d_safety [n_total]; d_waypoint_updated may be NULL.
 * lscqp_record_download    out [n_missions] and, if not NULL, agent_distance [n_total]; waits for the device.
 * lscqp_record_points      device pointer of float[n_total][n_samples][3]: the points of the last step (agents of finished missions keep the
 *                          points of the step that finished them).
 * lscqp_record_unfinished  the number of missions not yet finished (one 4-byte copy); waits for the device.
 * lscqp_plan_set_record    desc != NULL gives the plan a record of its own (NULL: takes it away), accumulated by the LAST node of the chain,
 *                          eager and captured.  Needs safety_samples > 0 and n_agents == n_total (LSCQP_ERR_INVALID_ARGUMENT says which
 *                          failed).  It may come before or after lscqp_plan_set_missions: the record is rebuilt for the partition in force
 *                          at lscqp_plan_reset, which must follow (a step before it is refused), requires goal_points -- they are the
 *                          desired goals, pinned to the mission's plane in 2-D like the states -- and clears the record.  A plan without a
 *                          record enqueues the chain it always did, node for node.
 * lscqp_plan_record        the plan's own record, NULL without one; owned by the plan.
 * lscqp_plan_run           flies the plan until every mission has finished: replans are enqueued in batches of check_every >= 1 (through the
 *                          graph if use_graph != 0), behind each batch the 4-byte count of unfinished missions is copied and waited for, and
 *                          the call returns at 0 or after max_replans.  Needs a record, closed_loop != 0 and waypoint_mode =
 *                          LSCQP_WAYPOINT_GRID_PIBT (nothing else flies without host writes between replans; LSCQP_ERR_INVALID_ARGUMENT
 *                          otherwise).  Because records freeze, the records do not depend on check_every; *replans_enqueued does. */
typedef struct lscqp_record_desc {
    double goal_threshold; /* param.goal_threshold, 0.1 in the launch files */
} lscqp_record_desc;
typedef struct lscqp_mission_record { /* 160 bytes */
    int32_t finished;               /* 1 = every agent was within goal_threshold of its goal at the start of replan `replans - 1` */
    int32_t replans;                /* replans accumulated (r + 1 after replan r); frozen when finished */
    int32_t first_qp_failed_replan; /* -1: none */
    int32_t reserved;
    double flight_time;             /* (replans - 1) * time_step once finished (total_flight_time), -1 until then */
    double distance;                /* total_flight_distance: sum of the agents' distances in id order (formed at the download) */
    double safety_ratio_agent;      /* +inf: nothing compared */
    int32_t safety_replan, safety_agent, safety_other, reserved2; /* replan, agent and other agent (global ids) attaining it; -1 */
    double vel_excess_ratio[3];     /* per-axis maxima; the summary prints their float norm() (:685-686) */
    double acc_excess_ratio[3];
    int64_t qp_failed, invalid, goal_failed, sfc_kept, waypoint_updates;
    int64_t max_in_range;
    int64_t truncated;
} lscqp_mission_record;
typedef struct lscqp_record_s* lscqp_record;
int lscqp_record_create(lscqp_handle h, int64_t n_total, int32_t n_missions, const int64_t* mission_offsets, int32_t n_samples,
                        double record_time_step, double time_step, double z_2d, const lscqp_record_desc* desc, lscqp_record* out);
void lscqp_record_destroy(lscqp_record rec);
int lscqp_record_reset(lscqp_record rec, const double* goal_points);
int lscqp_record_step_device(lscqp_record rec, const lscqp_header* d_hdr, const double* d_x_all, const int32_t* d_status,
                             const int32_t* d_goal_status, const int32_t* d_sfc_status, const int32_t* d_valid, const int32_t* d_in_range,
                             const lscqp_safety* d_safety, const int32_t* d_waypoint_updated, void* stream);
int lscqp_record_download(lscqp_record rec, lscqp_mission_record* out, double* agent_distance);
void* lscqp_record_points(lscqp_record rec, uint64_t* bytes_out);
int lscqp_record_unfinished(lscqp_record rec, int32_t* unfinished_out);
int lscqp_plan_set_record(lscqp_plan plan, const lscqp_record_desc* desc);
lscqp_record lscqp_plan_record(lscqp_plan plan);
int lscqp_plan_run(lscqp_plan plan, int64_t max_replans, int32_t check_every, int32_t use_graph, void* stream, int64_t* replans_enqueued);

/* ---- the flight log: every replan's sampled states kept on the device ------------------------------------------------------------------
 *
 * The reference's second file per mission is the result log (MultiSyncSimulator::saveSimulationResultAsCSV, src/multi_sync_simulator.cpp
 * :586-656): at every sample time of every replan each agent's position, velocity and acceleration and each obstacle's position and size;
 * its replayer reads that file.  The record's points buffer holds the last replan only, and a flight through lscqp_plan_run or a replayed
 * graph overwrites the plan buffer every replan.  A record with a log keeps every replan's rows: ONE more kernel (csrc/lscrecord.hip:
 * flight_log_kernel), enqueued in front of the record's own on the same stream.  It reads the record's replan counter before the record
 * increments it, so row r holds replan r; a thread owns one (agent, sample) pair and stores to that pair's slots alone -- no atomics, and
 * nothing the record's kernel reads or writes is written.  A mission that has finished is logged no further (its record is frozen, so are
 * its rows), and neither is one whose log is full: the record goes on counting, which is how overflow is told.
 *
 * Layout, mission-major so that one mission's log is one contiguous range.  off[] the partition, n_k = off[k+1] - off[k], S = n_samples,
 * C = max_replans, r the replan, a the GLOBAL agent id, s the sample:
 *   LSCQP_LOG_STATES     float  [ C*off[k]*S*9 + ((r*n_k + (a - off[k]))*S + s)*9 + {px,py,pz,vx,vy,vz,ax,ay,az} ]
 *                        Trajectory::getStateAt of the float32 control points at s * record_time_step (csrc/lscpost_traj.hpp: state_at;
 *                        axes >= dim: z_2d, at rest), float32 as State holds them.  The positions are the record's points, bit for bit.
 *   LSCQP_LOG_FLAGS      int32  [ C*off[k] + r*n_k + (a - off[k]) ]   LSCQP_LOG_FLAG_* : the five per-agent conditions the record counts
 *   LSCQP_LOG_OBSTACLES  float  [ ((k*C + r)*n_dyn + oi)*4 + {px,py,pz,radius} ]   the caller's table entry oi as it stands when the
 *                        replan's log is written (in a plan: as the replan's advance left it).  One entry per replan: the reference
 *                        logs the obstacle unchanged over a step's samples.
 * Row (r, s) stands at time r * time_step + s * record_time_step.  Rows at or beyond a mission's `rows` are unspecified.
 * lscqp_record_set_log        max_replans > 0 attaches a log of that capacity (zeroed once) with n_dyn >= 0 obstacle columns and no table;
 *                             0 removes it.  Waits for the device.  A failed call leaves the record as it was.  lscqp_record_reset
 *                             clears nothing of a log: rows restart at 0 because the counter does.  A record without a log enqueues
 *                             exactly what it always did.
 * lscqp_record_log_obstacles  the DEVICE table (borrowed, n_dyn entries) the obstacle columns are read from at every later step; NULL:
 *                             none are written.
 * lscqp_record_log            raw device pointer of one buffer (which = LSCQP_LOG_*) and its size, as lscqp_record_points.
 * lscqp_record_log_rows       rows[k] = min(replans, max_replans) and, if not NULL, overflowed[k] = replans > max_replans, per mission,
 *                             from the records; waits for the device.
 * lscqp_record_log_download   replans [first_replan, first_replan + n_replans) of one mission to the host: states [n_replans][n_k][S][9],
 *                             flags [n_replans][n_k], obstacles [n_replans][n_dyn][4]; any of the three may be NULL.  Waits for the
 *                             device.  LSCQP_ERR_INVALID_ARGUMENT where the range exceeds the mission's rows.
 * lscqp_plan_set_flight_log   max_replans > 0 gives the plan's record a log of that capacity (0: takes it away), with the plan's obstacle
 *                             columns and table -- lscqp_plan_set_obstacles may come before or after.  Needs a record
 *                             (lscqp_plan_set_record first; taking the record away takes the log with it).  lscqp_plan_reset must follow.
 *                             The chain gains one node, immediately in front of the record's, which stays the last.  Because missions
 *                             freeze, the log of a flight through lscqp_plan_run does not depend on check_every. */
#define LSCQP_LOG_STATES 0
#define LSCQP_LOG_FLAGS 1
#define LSCQP_LOG_OBSTACLES 2
#define LSCQP_LOG_COUNT 3
#define LSCQP_LOG_FLAG_QP_FAILED 1    /* QP status != LSCQP_STATUS_OPTIMAL */
#define LSCQP_LOG_FLAG_INVALID 2      /* valid == 0 */
#define LSCQP_LOG_FLAG_GOAL_FAILED 4  /* goal LP status != 0 */
#define LSCQP_LOG_FLAG_SFC_KEPT 8     /* sfc_status == 0 */
#define LSCQP_LOG_FLAG_WAYPOINT 16    /* waypoint updated (never set where the step has no such buffer) */
int lscqp_record_set_log(lscqp_record rec, int32_t max_replans, int32_t n_dyn);
int lscqp_record_log_obstacles(lscqp_record rec, const lscqp_obstacle* d_table);
void* lscqp_record_log(lscqp_record rec, int32_t which, uint64_t* bytes_out);
int lscqp_record_log_rows(lscqp_record rec, int32_t* rows, int32_t* overflowed);
int lscqp_record_log_download(lscqp_record rec, int32_t mission, int32_t first_replan, int32_t n_replans, float* states, int32_t* flags,
                              float* obstacles);
int lscqp_plan_set_flight_log(lscqp_plan plan, int32_t max_replans);

/* ---- the obstacle record: each mission's least agent-obstacle safety ratio over the whole flight -----------------------------------------
 *
 * The reference's summary line carries safety_ratio_obs, the minimum over the flight of the agent-obstacle safety ratio (MultiSyncSimulator::
 * update, src/multi_sync_simulator.cpp:527-557, written at :658-709).  lscqp_safety_obstacles_device forms the figure of ONE replan per agent;
 * a record that has been given those figures keeps their minimum per mission and per agent in a side buffer of its own: ONE more kernel
 * (csrc/lscrecord.hip: record_obstacles_kernel, one workgroup per mission), enqueued in front of the flight log's kernel where there is
 * one, otherwise in front of the record's own, on the same stream.  lscqp_mission_record itself is unchanged.
 * The kernel reads the record's `finished` word and replan counter before the record's kernel, behind it, sets and increments them: replan
 * r of a mission that has not finished is accumulated as r (the rule of the flight log), and a finished mission's figures are frozen with
 * its record -- its workgroup returns after loading one word.  At replan r, for every mission not finished, from the lscqp_safety_obs
 * [n_total] of the replan:
 *   - per agent a: its entry takes the replan's figure, with r and the figure's closest_obstacle and sample, where the figure is STRICTLY
 *     smaller than the entry's (an earlier replan keeps a tie; a NaN is never taken);
 *   - compared grows by the agents whose figure is finite, below_one by those whose figure is < 1.0 (strict; 1.0 itself is not counted);
 *   - the replan's minimum over the mission's agents, ties to the smallest agent id, replaces the mission's figure -- with r, that agent's
 *     GLOBAL id, its closest_obstacle and sample -- where it is STRICTLY smaller: the reference's `if (safety_ratio_obs > current)` applied in
 *     the order replan, then agent id, the order of safety_ratio_agent in the mission record.
 * No floating-point atomics: the result does not depend on how the agents fall onto lanes.
 * lscqp_record_set_obstacle_figures  d_safety_obs: DEVICE pointer [n_total], borrowed, read at every later lscqp_record_step_device; NULL removes
 *                                    the obstacle record (its figures with it).  The first use allocates the side buffer, cleared.  Waits
 *                                    for the device.  A failed call leaves the record as it was.  lscqp_record_reset clears the figures: ratios
 *                                    +inf, replan / agent / obstacle / sample -1, counts 0.  A record without obstacle figures enqueues
 *                                    exactly what it always did.
 * lscqp_record_obstacles_download    out [n_missions] and, if not NULL, agents [n_total] (global id order); waits for the device.
 *                                    LSCQP_ERR_INVALID_ARGUMENT where the record keeps no obstacle figures.
 * lscqp_record_obstacles_raw         raw device pointer of the side buffer and its size, as lscqp_record_points (NULL without obstacle figures):
 *                                    LSCQP_OBSREC_SPARE bytes, lscqp_mission_obstacle_record [n_missions], LSCQP_OBSREC_SPARE bytes,
 *                                    lscqp_agent_obstacle_record [n_total], LSCQP_OBSREC_SPARE bytes.  Nothing ever writes the spare bytes.
 * lscqp_plan_set_obstacle_record     on != 0 has the plan's record keep the obstacle figures of the plan's LSCQP_PLAN_OBS_SAFETY buffer (0: no
 *                                    longer).  Needs a record and obstacles (LSCQP_ERR_INVALID_ARGUMENT names the one that is missing); it may
 *                                    come before or after lscqp_plan_set_flight_log; taking the record or the obstacles away takes it away
 *                                    with them.  Waits for the device, drops a captured graph; lscqp_plan_reset must follow (a step before
 *                                    it is refused) and re-attaches the figures to the record of the partition in force.  The chain gains one
 *                                    node, in front of the log's or else the record's, which stays the last.  Because missions freeze, the
 *                                    obstacle record of a flight through lscqp_plan_run does not depend on check_every.  A plan that does not
 *                                    ask for it enqueues the chain it always did, node for node. */
#define LSCQP_OBSREC_SPARE 64
typedef struct lscqp_mission_obstacle_record { /* 40 bytes */
    double safety_ratio_obs;                 /* +inf: nothing compared (SP_INFINITY in the reference) */
    int32_t replan, agent, obstacle, sample; /* attaining it; -1: none.  agent is a GLOBAL id */
    int64_t below_one;                       /* agent-replans whose replan minimum was < 1.0 (strict) */
    int64_t compared;                        /* agent-replans with a finite figure */
} lscqp_mission_obstacle_record;
typedef struct lscqp_agent_obstacle_record { /* 24 bytes */
    double safety_ratio_obs;                 /* the agent's own running minimum, +inf */
    int32_t replan, obstacle, sample, reserved;
} lscqp_agent_obstacle_record;
int lscqp_record_set_obstacle_figures(lscqp_record rec, const lscqp_safety_obs* d_safety_obs);
int lscqp_record_obstacles_download(lscqp_record rec, lscqp_mission_obstacle_record* out, lscqp_agent_obstacle_record* agents);
void* lscqp_record_obstacles_raw(lscqp_record rec, uint64_t* bytes_out);
int lscqp_plan_set_obstacle_record(lscqp_plan plan, int32_t on);

/* ---- dynamic obstacles in the chain: their motion on the device, their rows and their safety figures ------------------------------------
 *
 * The reference's missions list dynamic obstacles (mission file "obstacles": spin, straight, patrol, chasing, gaussian, real; include/
 * obstacle.hpp).  ObstacleGenerator::update(t, 0) moves them once per replan, at the replan's start time and without observer noise
 * (src/multi_sync_simulator.cpp:311); broadcastMsgs hands EVERY agent all of them, unfiltered, in front of the in-range agents (:310-333);
 * their LSC rows are hard rows like an agent's (CollisionConstraints::dynamic_obstacle_indices is never filled); the safety figures of
 * the replan read the same positions (:527-557); planMAPF's grid does not see them.
 * A model describes how ONE obstacle moves; `kind` selects the reference class:
 *   LSCQP_OBSTACLE_STRAIGHT  StraightObstacle (:138-214): start -> goal under a trapezoidal speed profile (speed, max_acc), both branches
 *                            (dist_to_goal > 2 dist_acc, and the short one) with their phases; past the last phase the obstacle rests
 *                            at the goal with zero velocity.  Reads start, goal.
 *   LSCQP_OBSTACLE_PATROL    PatrolObstacle (:216-264): n_waypoints <= LSCQP_OBSTACLE_MAX_WAYPOINTS legs flown as straight obstacles one
 *                            after the other, the last leg back to waypoint 0, for ever.  Reads waypoints.  Whole laps are taken off
 *                            the time first and at most n_waypoints legs are walked, whatever the time (the reference subtracts leg by
 *                            leg from t = 0): equal in the first lap, within rounding of the lap time afterwards.
 *   LSCQP_OBSTACLE_SPIN      SpinObstacle (:83-136): `start` rotated about the axis (axis_point, axis_direction) at angular speed
 *                            speed / spin radius, in double; the velocity is the position's offset turned by 90 degrees about the axis
 *                            times the angular speed, as the reference forms it.
 *   LSCQP_OBSTACLE_HELD      lscqp_obstacles_advance_device leaves the table entry alone.  Without a drive ("chasing and gaussian
 *                            obstacles" below) the caller writes position and velocity between eager replans (real obstacles; chasing
 *                            and gaussian ones played on the host); with a drive the entry is moved on the device, in front of the
 *                            advance.  `start` is where the entry is put by lscqp_plan_set_obstacles / lscqp_plan_reset.
 * Positions and velocities are point3d in the reference: the kernel writes float32 values held in double, formed with the reference's
 * own mix of float and double operations and without fused multiply-adds.
 * lscqp_obstacle_model_prepare   HOST, no device needed: checks n models and fills their derived fields in place -- per leg the
 *                            direction, dist_to_goal, dist_acc and flight_time of StraightObstacle's constructor in its own arithmetic
 *                            (Vector3::distance and normalized() on float32 points), the lap time, the spin's unit axis, offset and
 *                            angular speed.  LSCQP_ERR_INVALID_ARGUMENT names the model and what is wrong with it: an unknown kind, a
 *                            non-finite field, radius < 0, max_acc <= 0, speed <= 0 (not asked of a HELD model), n_waypoints outside
 *                            [1, LSCQP_OBSTACLE_MAX_WAYPOINTS], a patrol whose lap time is not positive (a lap of no length would never
 *                            end in the reference either), a spin whose axis direction or spin radius is zero.
 * lscqp_obstacles_advance_device one launch of ONE workgroup over n_dyn <= lscqp_max_obstacles(h) PREPARED models in device memory:
 *                            reads the obstacle clock r (int32, device) and forms t as the reference's clock does -- r steps of
 *                            ros::Duration(time_step), whole nanoseconds, then seconds -- writes entry oi of d_obstacles (position,
 *                            velocity, radius, downwash, max_acc, type = DYNAMICOBSTACLE) for every model that is not HELD, and stores
 *                            r + 1.  The clock lives on the device because a captured graph carries constant arguments.
 * lscqp_plan_set_obstacles   gives the plan n_dyn obstacles (host models, prepared by the call itself; the caller's array is not
 *                            written) and the generator's parameters; n_dyn = 0 or models = NULL takes them away.  Like
 *                            lscqp_plan_set_record it waits for the device and drops a captured graph, lscqp_plan_reset must follow (a step
 *                            before it is refused) and the reset puts the table at t = 0 and zeroes the clock.  desc.n_obs stays the
 *                            number of row slots per agent: slots [0, n_dyn) are the obstacles in table order, slots [n_dyn, n_obs) the
 *                            in-range agents (the range filter then cuts to the n_obs - n_dyn nearest).  Refused, leaving the plan as
 *                            it was: n_dyn > n_obs (LSCQP_ERR_INVALID_ARGUMENT), constraint_mode LSCQP_GEN_BVC (LSCQP_ERR_UNSUPPORTED:
 *                            the obstacle rows are generateLSC's or generateCLSC's), a model lscqp_obstacle_model_prepare refuses.
 *                            Per replan the chain gains, on its one stream: the advance in front of the prepare step, the obstacle
 *                            rows of the plan's constraint_mode over the planning agents' initial trajectories behind the agent rows
 *                            (LSCQP_GEN_LSC: lscqp_generate_lsc_obstacles_device; LSCQP_GEN_CLSC: lscqp_generate_obstacle_rows_device
 *                            in that mode without obstacle goal points, i.e. the origin, as in the reference -- the goal LP reads the
 *                            last-segment rows of every slot, the obstacles' too), and with safety_samples > 0
 *                            lscqp_safety_obstacles_device behind the agent safety figures.  A mission
 *                            partition shares THIS table like the map (a table per mission: lscqp_plan_set_mission_obstacles, "a mission's
 *                            own obstacles" below); every owner of a sharded mission advances its own copy of the same table.  The waypoint decision does not see obstacles, as in the reference.  The mission record keeps
 *                            no obstacle figure itself; the obstacle record beside it does (lscqp_plan_set_obstacle_record).
 * lscqp_plan_obstacle_buffer / _upload / _download   the buffers that exist only with obstacles (NULL and 0 bytes otherwise), addressed
 *                            by LSCQP_PLAN_OBS_*; copies are synchronous like lscqp_plan_upload / _download. */
#define LSCQP_OBSTACLE_MAX_WAYPOINTS 8
#define LSCQP_OBSTACLE_HELD 0 /* values of lscqp_obstacle_model.kind (lscqp_obstacle.type is another field: 0 = DYNAMICOBSTACLE) */
#define LSCQP_OBSTACLE_STRAIGHT 1
#define LSCQP_OBSTACLE_PATROL 2
#define LSCQP_OBSTACLE_SPIN 3
typedef struct lscqp_obstacle_leg { /* StraightObstacle's members; 64 bytes */
    float start[3], goal[3], n[3]; /* point3d */
    float reserved;
    double dist_to_goal, dist_acc, flight_time;
} lscqp_obstacle_leg;
typedef struct lscqp_obstacle_model { /* 912 bytes */
    int32_t kind;        /* LSCQP_OBSTACLE_* */
    int32_t n_waypoints; /* PATROL */
    double radius, downwash, max_acc, speed; /* mission file: size, downwash, max_acc, speed */
    double start[3], goal[3];                /* STRAIGHT; start also SPIN and HELD */
    double waypoints[LSCQP_OBSTACLE_MAX_WAYPOINTS][3];
    double axis_point[3], axis_direction[3]; /* SPIN: axis.pose.position, axis.pose.orientation x y z */
    /* derived, filled by lscqp_obstacle_model_prepare */
    int32_t n_legs, prepared;
    lscqp_obstacle_leg leg[LSCQP_OBSTACLE_MAX_WAYPOINTS];
    double lap_time;                                   /* flight_time[0] + flight_time[1] + ... in that order */
    double spin_axis[3], spin_offset[3], spin_w;       /* n, a = start - axis_point, w = speed / |a - (a.n) n| */
} lscqp_obstacle_model;
int lscqp_obstacle_model_prepare(lscqp_obstacle_model* models, int32_t n);
int lscqp_obstacles_advance_device(lscqp_handle h, const lscqp_obstacle_model* d_models, int32_t n_dyn, double time_step, int32_t* d_clock,
                                   lscqp_obstacle* d_obstacles, void* stream);
#define LSCQP_PLAN_OBS_TABLE 0  /* i/o  lscqp_obstacle[n_dyn]: the table as the last replan's advance left it (HELD entries: the caller's); a
                                        table per mission: [n_dyn_total], mission-major */
#define LSCQP_PLAN_OBS_SAFETY 1 /* out  lscqp_safety_obs[n_agents] of the last replan (safety_samples > 0) */
#define LSCQP_PLAN_OBS_CLOCK 2  /* i/o  int32: the replan index the NEXT advance evaluates; a table per mission: int32[n_missions] */
#define LSCQP_PLAN_OBS_COUNT 3
int lscqp_plan_set_obstacles(lscqp_plan plan, const lscqp_obstacle_param* param, int32_t n_dyn, const lscqp_obstacle_model* models);
void* lscqp_plan_obstacle_buffer(lscqp_plan plan, int32_t which, uint64_t* bytes_out);
int lscqp_plan_obstacle_upload(lscqp_plan plan, int32_t which, const void* host, uint64_t offset, uint64_t bytes);
int lscqp_plan_obstacle_download(lscqp_plan plan, int32_t which, void* host, uint64_t offset, uint64_t bytes);

/* ---- chasing and gaussian obstacles: the two models whose next state needs more than the time -------------------------------------------
 *
 * ChasingObstacle (include/obstacle.hpp:267-364) accelerates towards a goal point and away from the other obstacles as the previous update
 * left them; GaussianObstacle (:366-469) integrates a history of accelerations, one per acc_update_cycle.  Both stay LSCQP_OBSTACLE_HELD
 * models -- the advance does not touch them -- and get a DRIVE: one more record per obstacle, in a table beside the models, and one more
 * kernel in front of the advance that moves every driven entry by one replan.  Radius, max_acc, downwash and `start` are the model's.
 *   LSCQP_DRIVE_NONE      no drive: the entry is the caller's, as ever.
 *   LSCQP_DRIVE_CHASING   getChasingObstacle (:313-363), ONE update per replan with dt = t(r) - t(r - 1) of the obstacle clock r (0 at r = 0:
 *                         t_last_called starts at 0): a = gamma_target (goal - position); over the OTHER table entries in table order, as
 *                         the previous replan left them, skipping those closer than 1e-5, the repulsion term of :336-337 inside
 *                         Q* = 2 (radius + other.radius); |a| clamped to max_acc - 0.01; v += a dt; |v| clamped to max_vel;
 *                         position += v dt, narrowed to float.  The goal point is the position of global agent target_agent in the state
 *                         buffer at the replan's start (target_agent >= 0) or goal[3] (target_agent = -1; the origin is what the
 *                         reference's own simulator passes, include/obstacle_generator.hpp:28-32).  The entry's own previous position
 *                         and velocity are read from the table.  All entries are read before any is written (a Jacobi step).
 *   LSCQP_DRIVE_GAUSSIAN  getGaussianObstacle (:424-468): the loop over i = 0 .. n, n = floor((t + 1e-5) / acc_update_cycle), with both
 *                         branches of its max_vel test, over the slice [history_first, history_first + history_len) of ONE shared table of
 *                         accelerations (double[3] each; GaussianObstacle::set_acc_history).  The state after i_done whole cycles is kept
 *                         in a checkpoint per obstacle, advanced to n, and the partial step dt = t - n cycle is taken on a copy: the whole
 *                         cycles of the reference's loop do not depend on t, so this is the loop from zero bit for bit at the cost of the
 *                         cycles since the last replan.  A checkpoint ahead of the clock (i_done > n: the caller wrote the clock
 *                         backwards) restarts from `start`.  Past the end of its slice the obstacle accelerates by zero and bit 0 of its
 *                         table entry's `reserved` word is set (LSCQP_OBSTACLE_HISTORY_ENDED); the reference draws new accelerations there.
 * Positions and velocities are point3d: float32 held in double, narrowed exactly where the reference stores into one.  The norm of an
 * Eigen::Vector3d is sqrt((x x + y y) + z z) here (Eigen's own order depends on its version and vectorisation); nothing contracts a multiply
 * and an add; only + - x / sqrt are used.  broadcastMsgs' repeats of the update with dt = 0, once per agent, are not made.
 * lscqp_obstacle_drive_check     HOST, no device needed: n drives against their n models, a history table of n_history entries and a
 *                            mission of n_total agents.  LSCQP_ERR_INVALID_ARGUMENT names the model and the cause: a drive on a model that
 *                            is not HELD, an unknown kind, a non-finite field, max_vel <= 0, acc_update_cycle <= 0 (GAUSSIAN), a history
 *                            slice of length 0 or outside [0, n_history) (GAUSSIAN), target_agent outside [-1, n_total) (CHASING),
 *                            max_acc <= 0.01 (CHASING: the clamp is to max_acc - 0.01).
 * lscqp_obstacles_drive_device   one launch of ONE workgroup over n_dyn <= lscqp_max_obstacles(h) models and drives in device memory, IN
 *                            FRONT of lscqp_obstacles_advance_device on the same stream: reads the clock r (forms t(r) and t(r - 1) as the
 *                            advance forms t; does not write it), moves every entry whose drive is not NONE and writes its radius,
 *                            downwash, max_acc, type = DYNAMICOBSTACLE and `reserved`.  d_state [n_total][9] is LSCQP_PLAN_BUF_STATE's layout
 *                            (may be NULL with n_total = 0: every chaser then flies to goal[3]); d_drive_state one checkpoint per obstacle,
 *                            zeroed by the caller before the first replan (GAUSSIAN only); d_acc_history may be NULL with n_history = 0.
 *                            An index outside its table is never followed: such a target reads goal[3], such an acceleration is zero.
 * lscqp_obstacle_drive_host      the same arguments as HOST pointers, one replan on the CPU by the same functions the kernel runs: no device
 *                            needed.  (The clock is read, not written: the caller advances it, or runs the advance's restatement.)
 * lscqp_plan_set_obstacle_drives gives the plan's n_dyn obstacles their drives (host arrays, copied and checked by
 *                            lscqp_obstacle_drive_check against the plan's models and n_total; n_dyn must be the plan's); drives = NULL or
 *                            n_dyn = 0 takes them away, and so does every lscqp_plan_set_obstacles.  Like the other setters it waits for the
 *                            device and drops a captured graph, lscqp_plan_reset must follow (a step before it is refused), a refused call
 *                            leaves the plan as it was; the reset puts driven entries at `start` with zero velocity and zeroes the
 *                            checkpoints.  Per replan the chain gains exactly one node, in front of the advance; a plan without drives
 *                            enqueues the chain it always did node for node.  target_agent is a global agent index: a mission partition
 *                            shares driven obstacles like any other, and every owner of a sharded mission drives its own copy.  With a
 *                            table per mission (below) n_dyn is the tables' total, the node is lscqp_obstacles_drive_missions_device, and
 *                            a chaser whose target_agent (>= 0) is not an agent of the mission that owns the chaser is refused, at the call
 *                            and again at the reset (the partition's offsets may have moved). */
#define LSCQP_DRIVE_NONE 0
#define LSCQP_DRIVE_CHASING 1
#define LSCQP_DRIVE_GAUSSIAN 2
#define LSCQP_OBSTACLE_HISTORY_ENDED 1 /* bit 0 of lscqp_obstacle.reserved of a GAUSSIAN entry */
typedef struct lscqp_obstacle_drive { /* 96 bytes */
    int32_t kind;                     /* LSCQP_DRIVE_* */
    int32_t target_agent;             /* CHASING: global agent id, or -1 = goal[3] */
    double max_vel;                   /* mission file: max_vel (both kinds) */
    double gamma_target, gamma_obs;   /* CHASING */
    double goal[3];                   /* CHASING with target_agent = -1 */
    double initial_vel[3];            /* GAUSSIAN (held as point3d) */
    double acc_update_cycle;          /* GAUSSIAN */
    int32_t history_first, history_len; /* GAUSSIAN: its slice of the acceleration table */
} lscqp_obstacle_drive;
typedef struct lscqp_obstacle_drive_state { /* 56 bytes: a GAUSSIAN obstacle after i_done whole cycles; all zero = at `start` */
    int32_t i_done, reserved;
    float position[3], velocity[3]; /* gaussianObstacle.position / .velocity */
    double v[3];                    /* the loop's v */
} lscqp_obstacle_drive_state;
int lscqp_obstacle_drive_check(const lscqp_obstacle_model* models, const lscqp_obstacle_drive* drives, int32_t n, int32_t n_history,
                               int64_t n_total);
int lscqp_obstacles_drive_device(lscqp_handle h, const lscqp_obstacle_model* d_models, const lscqp_obstacle_drive* d_drives, int32_t n_dyn,
                                 const double* d_acc_history, int32_t n_history, const double* d_state, int64_t n_total,
                                 lscqp_obstacle_drive_state* d_drive_state, double time_step, const int32_t* d_clock,
                                 lscqp_obstacle* d_obstacles, void* stream);
int lscqp_obstacle_drive_host(lscqp_handle h, const lscqp_obstacle_model* models, const lscqp_obstacle_drive* drives, int32_t n_dyn,
                              const double* acc_history, int32_t n_history, const double* state, int64_t n_total,
                              lscqp_obstacle_drive_state* drive_state, double time_step, const int32_t* clock, lscqp_obstacle* obstacles,
                              void* stream);
int lscqp_plan_set_obstacle_drives(lscqp_plan plan, const lscqp_obstacle_drive* drives, int32_t n_dyn, const double* acc_history,
                                   int32_t n_history);

/* ---- a mission's own obstacles: one obstacle table per mission of a partition -------------------------------------------------------------
 *
 * The reference flies one mission file at a time and every file lists its own obstacles.  A partition of K missions (lscqp_plan_set_missions)
 * that shares one table would hand every agent the obstacles of every mission, let a chaser of one mission fly through all of them, and
 * spend a row slot of every agent on every obstacle of every mission.  Here the table is MISSION-MAJOR: mission k owns the entries
 * [obstacle_offsets[k], obstacle_offsets[k + 1]) of the models, the drives, the checkpoints and the table, and one clock word, clock[k].
 * obstacle_offsets has n_missions + 1 int32 values, non-decreasing from 0 to n_dyn_total; a mission may own no obstacle.  The device entries
 * take the list twice, like the *_missions_device entries take the partition: on the host, checked before the device is touched
 * (LSCQP_ERR_INVALID_ARGUMENT: not from 0, decreasing, last != n_dyn_total; LSCQP_ERR_UNSUPPORTED: one mission's count above
 * lscqp_max_obstacles(h) -- the TOTAL is not bounded by it), and on the device, where the kernels read it.  n_missions = 0 is the empty batch.
 * lscqp_obstacles_advance_missions_device   lscqp_obstacles_advance_device with one workgroup per mission over its slice, by the same
 *                            functions: workgroup k reads clock[k] in front of its barrier and stores clock[k] + 1 behind it (one word could
 *                            not be read by K workgroups and counted by one of them without a race).  A mission without obstacles still
 *                            counts its clock; with n_dyn_total = 0 the models and the table may be NULL.
 * lscqp_obstacles_drive_missions_device     lscqp_obstacles_drive_device with one workgroup per mission, IN FRONT of the advance: it stages its
 *                            own slice only (dynamic LDS: the largest mission's count of 32-byte records), so a chaser is repelled by the
 *                            obstacles of its own mission and no other; target_agent stays a global index into d_state, the history table
 *                            is one for all missions.  Reads clock[k], does not write it.
 * lscqp_safety_obstacles_ids_device         lscqp_safety_obstacles_device in which local agent a is judged against the entries named by row a
 *                            of d_obstacle_ids [n_agents][n_slots]: table indices, those outside [0, n_obstacles) -- -1 by convention --
 *                            skipped, type REAL skipped as ever.  Samples, then slots, strict <: the first (sample, slot) attaining the
 *                            minimum; closest_obstacle is the SLOT, which is the index a plan of that mission alone reports.  Nothing
 *                            compared: +inf, -1, -1.  The arithmetic is the other entry's, bit for bit.
 * lscqp_plan_set_mission_obstacles   gives mission k of the partition IN FORCE its own obstacles: models [obstacle_offsets[n_missions]] in
 *                            mission order (host, prepared by the call; the caller's array is not written).  The lifecycle is
 *                            lscqp_plan_set_obstacles': it waits for the device and drops a captured graph, lscqp_plan_reset must follow (a
 *                            step before it is refused), the reset puts every entry at t = 0 and zeroes all K clocks, a refused call leaves
 *                            the plan as it was.  It and lscqp_plan_set_obstacles replace each other; n_missions = 0, models = NULL or
 *                            missions none of which owns an obstacle take the obstacles away.  Row slots: n_slot = the largest mission's
 *                            count, n_slot <= desc.n_obs required; slot o < n_slot of an agent of mission k holds entry obstacle_offsets[k]
 *                            + o for o < count_k and nothing (all-zero rows, which bind nothing) beyond; slots [n_slot, n_obs) hold the
 *                            in-range agents.  Refused: n_missions other than the partition's (LSCQP_ERR_INVALID_ARGUMENT; a later
 *                            lscqp_plan_set_missions with another count is refused while these obstacles are set, as with worlds; the reset
 *                            makes each agent's list again from the offsets then in force); a sharded plan (n_agents != n_total);
 *                            constraint_mode LSCQP_GEN_BVC (LSCQP_ERR_UNSUPPORTED); together with a flight log, in either order
 *                            (LSCQP_ERR_UNSUPPORTED: the log's obstacle columns are those of one shared table).  Per replan the chain has
 *                            exactly the nodes of a plan with a shared table: the three entries above and the row entries called with
 *                            n_slot and the agents' own lists.  (A plan keeps a shared table as the one-table case of this layout --
 *                            offsets {0, n_dyn}, one clock word, every agent's list 0 .. n_dyn - 1 -- and moves it by the same entries;
 *                            each of the three is one kernel text with its shared form, obstacle_advance_kernel<MIS>,
 *                            obstacle_drive_kernel<MIS> and safety_obstacles_kernel<IDS>.)  lscqp_plan_set_obstacle_drives,
 *                            lscqp_plan_set_obstacle_record (its `obstacle` is then the slot), lscqp_plan_run, worlds and a patrol compose
 *                            unchanged.  LSCQP_PLAN_OBS_TABLE is [n_dyn_total], LSCQP_PLAN_OBS_CLOCK int32[n_missions].  A plan that never
 *                            makes this call has the nodes, buffers and results it always had. */
int lscqp_obstacles_advance_missions_device(lscqp_handle h, const lscqp_obstacle_model* d_models, int32_t n_missions,
                                            const int32_t* obstacle_offsets, const int32_t* d_obstacle_offsets, int32_t n_dyn_total,
                                            double time_step, int32_t* d_clock, lscqp_obstacle* d_obstacles, void* stream);
int lscqp_obstacles_drive_missions_device(lscqp_handle h, const lscqp_obstacle_model* d_models, const lscqp_obstacle_drive* d_drives,
                                          int32_t n_missions, const int32_t* obstacle_offsets, const int32_t* d_obstacle_offsets,
                                          int32_t n_dyn_total, const double* d_acc_history, int32_t n_history, const double* d_state,
                                          int64_t n_total, lscqp_obstacle_drive_state* d_drive_state, double time_step,
                                          const int32_t* d_clock, lscqp_obstacle* d_obstacles, void* stream);
int lscqp_safety_obstacles_ids_device(lscqp_handle h, int64_t n_agents, int64_t first_agent, int64_t n_total, int32_t n_samples,
                                      double record_time_step, double z_2d, const double* d_x_all, const double* d_radius,
                                      const double* d_downwash, int32_t n_slots, const int32_t* d_obstacle_ids, int32_t n_obstacles,
                                      const lscqp_obstacle* d_obstacles, lscqp_safety_obs* d_out, void* stream);
int lscqp_plan_set_mission_obstacles(lscqp_plan plan, const lscqp_obstacle_param* param, int32_t n_missions, const int32_t* obstacle_offsets,
                                     const lscqp_obstacle_model* models);

/* ---- patrol missions: start and goal swapped on arrival, on the device ------------------------------------------------------------------
 *
 * With multisim/patrol set the reference's simulator runs in PlannerState::PATROL (src/multi_sync_simulator.cpp:57-61), isFinished never
 * ends the flight (:401-404), and every agent, at the top of its own plan(), swaps desired_goal_point and start_point as soon as
 *   desired_goal_point.distance(current_state.position) < param.goal_threshold        (AgentManager::planningStateTransition,
 *                                                                                      src/agent_manager.cpp:225-240).
 * The distance is the one the mission record's finish test forms (float32 differences of the position as the state buffer holds it --
 * z := (float)z_2d in a 2-D class -- and of the goal narrowed to float32; float32 sum of squares, nothing contracted; the square root in
 * double), compared in double with a STRICT <.  The record's test is `>`: at exact equality a GOTO mission is finished and a patrolling
 * agent does not turn.  A threshold of 0 is legal and never turns anyone.
 * lscqp_patrol_device          the transition alone, one thread per agent of d_state [n][9] (LSCQP_PLAN_BUF_STATE's layout): where the test
 *                          passes, d_desired[a] and d_start[a] ([n][3] doubles) are exchanged in place, d_legs[a] is incremented and
 *                          d_swapped[a] = 1; elsewhere d_swapped[a] = 0 -- the word is written on every call.  Asynchronous on `stream`,
 *                          capturable; dim is the class's 2 or 3.
 * lscqp_patrol_host            the same arguments as HOST pointers, one call on the CPU by the function the kernel runs: no device needed.
 * lscqp_patrol_check           HOST, no device needed: what lscqp_plan_set_patrol refuses -- a threshold that is negative or not finite, a
 *                          sharded plan (n_agents != n_total: the rule of safety_samples) -- with the cause named.
 * lscqp_field_exchange_device  for every agent with d_swapped[a] == 1 the agent's slice [a * nodes, (a + 1) * nodes) of d_field is exchanged
 *                          with the same slice of d_field_other, word by word, and d_init_d[a] with d_init_d_other[a]; every other word
 *                          is left alone.  One launch over (agent, chunk of 1024 nodes), dword accesses only.
 * lscqp_plan_set_patrol        the plan flies a patrol; NULL takes it away.  Like the other setters it waits for the device, drops a captured
 *                          graph and invalidates the distance fields; lscqp_plan_reset must follow (a step before it is refused by name);
 *                          a refused call leaves the plan as it was.  closed_loop = 0 is not refused: the caller writes the states, as
 *                          always.  The reset needs the goal points, puts every agent on leg 0 and zeroes LEGS and SWAPPED.
 * THE ORDER (one rule).  The reference's loop is decentralizedMAPP over the OLD goals, then per agent the transition, then
 * TrajPlanner::plan.  So the transition node sits directly behind the waypoint decision and in front of the obstacles' motion and
 * `prepare`; in waypoint_mode = LSCQP_WAYPOINT_GRID_PIBT the exchange node follows it directly.  That is exactly two more nodes per replan
 * with a grid and one without; a plan without patrol enqueues the chain it always did, node for node and argument for argument.
 * WHICH BUFFERS.  Grid mode: LSCQP_PLAN_BUF_DESIRED_GOAL and the plan's start points themselves.  At the reset the plan computes BOTH legs'
 * distance fields with the entries it always used (a second call with starts and goals exchanged: the same nodes are cleared, the mission
 * occupancy is the same; one more field per agent), and an agent that turns gets the other field and init_d by the exchange -- the
 * decision kernels read the active field where they always did.  A map that moves under the mission rebuilds the active field from
 * (start, desired) as they stand and the other from the exchanged pair, whatever legs the agents are on.  Static goals (optimize_goal = 0,
 * waypoint_mode = 0): LSCQP_PLAN_BUF_GOAL is the desired goal (goalPlanningWithStaticGoal) and a start buffer of the patrol's own is filled at
 * the reset.  Caller's waypoints with the goal LP (optimize_goal = 1, waypoint_mode = 0): desired and start buffers of the patrol's own,
 * for the caller's planner to read.  A mission partition and worlds compose (the field entries are the ones already used); obstacles and
 * their drives are untouched.  A plan with a record AND a patrol resets its record with desired goals at +infinity: every distance is
 * +inf, no mission ever finishes, lscqp_plan_run flies to max_replans.
 * lscqp_plan_patrol_buffer     the patrol's state (device pointers, NULL and 0 bytes where the plan has none: no patrol, or a FIELD entry
 *                          without a grid). */
typedef struct lscqp_patrol_desc { /* 8 bytes */
    double goal_threshold;         /* param.goal_threshold: the launch files' 0.1 */
} lscqp_patrol_desc;
#define LSCQP_PATROL_DESIRED 0      /* double[n_total][3]: the desired goals the transition swaps (grid mode: LSCQP_PLAN_BUF_DESIRED_GOAL itself) */
#define LSCQP_PATROL_START 1        /* double[n_total][3]: the start points */
#define LSCQP_PATROL_LEGS 2         /* int32[n_total]: legs completed since the reset */
#define LSCQP_PATROL_SWAPPED 3      /* int32[n_total]: 1 where the last replan's transition turned the agent */
#define LSCQP_PATROL_FIELD 4        /* int32[n_total][nodes]: the active distance fields (grid mode) */
#define LSCQP_PATROL_INIT_D 5       /* int32[n_total] */
#define LSCQP_PATROL_FIELD_OTHER 6  /* ... and those of the opposite leg */
#define LSCQP_PATROL_INIT_D_OTHER 7
#define LSCQP_PATROL_COUNT 8
int lscqp_patrol_check(const lscqp_patrol_desc* desc, int64_t n_agents, int64_t n_total);
int lscqp_patrol_device(lscqp_handle h, int64_t n, const double* d_state, double* d_desired, double* d_start, double goal_threshold, int32_t dim,
                        double z_2d, int32_t* d_legs, int32_t* d_swapped, void* stream);
int lscqp_patrol_host(lscqp_handle h, int64_t n, const double* state, double* desired, double* start, double goal_threshold, int32_t dim,
                      double z_2d, int32_t* legs, int32_t* swapped, void* stream);
int lscqp_field_exchange_device(int64_t n, int64_t nodes, const int32_t* d_swapped, int32_t* d_field, int32_t* d_field_other, int32_t* d_init_d,
                                int32_t* d_init_d_other, void* stream);
int lscqp_plan_set_patrol(lscqp_plan plan, const lscqp_patrol_desc* desc);
void* lscqp_plan_patrol_buffer(lscqp_plan plan, int32_t which, uint64_t* bytes_out);

/* ---- work counters of a launch (the fp64-VALU figure next to the HBM one) -----------------------------
 *
 * The kernel is bound by fp64 vector issue, not by HBM; the figure that goes with that roof is
 * "iterations x flops per iteration".  The iterations are the kernel's own count (lscqp_info.iterations, per instance); the flops
 * of one pass through the iteration body are a property of the kernel instance's machine code and are read off it when the library
 * is built (lsc_dr_planner_amd/isa_work.py: fp64 vector instructions between the position markers of the loop body; FMA = 2 flops
 * per lane, any other fp64 arithmetic instruction 1; x 64 lanes x wavefronts per instance).  lscqp_instance_work reports them for
 * the instance a launch of n QPs with n_obs_max obstacles selects -- the same selection lscqp_solve_batch_device makes.
 *   flops of an instance that ran `it` iterations  =  flops_fixed + it * flops_per_iteration + flops_last_pass
 * (the pass that detects convergence runs the residual pass and the test only).  These are the lane-flops the SIMDs EXECUTE,
 * masked lanes and the in-line blocks most iterations skip included (about 15 % above the hardware's own SQ_INSTS_VALU_*_F64
 * count, profiles/), i.e. an upper bound of the useful work and the quantity the 78.6 TFLOP/s fp64 vector peak of MI355X is about.
 * Regions of the nested-dissection instances that only one or two of the workgroup's wavefronts execute are counted for those
 * wavefronts only (the source brackets them with position markers). */
typedef struct lscqp_work {
    double flops_fixed;              /* prologue + epilogue */
    double flops_per_iteration;
    double flops_last_pass;
    double f64_insts_per_iteration;  /* per wavefront (averaged over the workgroup's wavefronts where they run different code) */
    double valu_insts_per_iteration; /* per wavefront, all vector-ALU instructions */
    double lds_insts_per_iteration;  /* per wavefront */
    double valu_insts_fixed;         /* per wavefront: prologue + epilogue + last pass */
    int32_t wavefronts;              /* per QP */
    int32_t nslot;                   /* LSC row slots per lane */
    int32_t max_obstacles;           /* capacity of the instance */
    int32_t lds_bytes;               /* per workgroup */
    char kernel[96];                 /* "lscqp_pdip_kernel<M,DIM,ES,NSLOT,W,FT>" */
} lscqp_work;
int lscqp_instance_work(lscqp_handle h, int64_t n, int32_t n_obs_max, lscqp_work* out);

/* ---- failure diagnostics (the reference's answer to a failed QP) -----------------------------------------------------------
 *
 * When CPLEX fails the reference exports the model as an LP file and runs the conflict refiner to NAME the rows that cannot hold
 * together (src/traj_optimizer.cpp:103-137; :45-52 with param.log_solver), and its caller prints every SFC / LSC row that the
 * fallback trajectory `initial_traj` violates, with obstacle, segment, control point and margin (src/traj_planner.cpp:767-797).
 *   lscqp_diagnose[_device]  evaluates every row of the reference's model (populatebyrow, src/traj_optimizer.cpp:238-511) on the
 *                            trajectories x [n][nv] (reference variable order, world frame): per row family the largest violation
 *                            (<= 0: satisfied, then the smallest margin negated) and the number of rows violated by more than `tol`,
 *                            plus the most violated row by name.  On initial_traj it IS the caller's debug loop; on the x_out of a
 *                            non-OPTIMAL instance (the iterate the solver stopped at) it names the rows that instance cannot satisfy.
 *                            Units are the reference's: metres for bounds / SFC / LSC (normal-weighted) / communication rows,
 *                            m/s and m/s^2 for the dynamic limits, the row's own scaling for the equalities.
 *                            A two-sided limit (bounds, corridor faces of one axis, |v|, |a|, communication rows) is ONE row with
 *                            one name; its violation is the larger of its two sides.  A row is counted when violation > tol, strictly.
 *                            Names (family, obstacle, segment, point, axis), -1 where a field does not apply:
 *                              BOUND, SFC            (-1, m, i, k)   control point i of segment m, axis k
 *                              LSC                   (oi, m, i, -1)  obstacle slot oi; a row with |n| < 1e-5 does not exist (:409-411)
 *                              VEL, ACC              (-1, m, i, k)   the difference that starts at control point i
 *                              COMM_PAIR             (mi, m, 5, k)   |c[m][5] - c[mi][0]|, mi <= m
 *                              COMM_WAYPOINT         (-1, m, 5, k)
 *                              EQUALITY              (-1, 0, j, k)   initial position / velocity / acceleration, j = 0 / 1 / 2
 *                                                    (-1, m, j, k)   m >= 1: the C0 / C1 / C2 join of segment m - 1 to m, j = 0 / 1 / 2
 *                                                    (-1, M-1, 4 | 3, k)  the end stop c5 = c4, c5 = c3 (LSC planner mode)
 *                            TIES.  Among rows of equal violation the named row is the least in (family, obstacle, segment, point,
 *                            axis), compared lexicographically -- e.g. a corridor face that coincides with a world face names BOUND.
 *                            NON-FINITE INPUT.  A row whose value is NaN or +inf cannot be shown to hold: it counts as violated, its
 *                            family's `worst` is +inf, and the named row is the least such row by the tie rule with violation = +inf.
 *                            That holds wherever the NaN enters: a control point, a header field, an LSC row, or ONE face of a
 *                            corridor or of the world box (a two-sided row is NaN if either side is).
 *                            The instances of a batch do not affect each other.
 *   lscqp_dump_instance      one instance as a CPLEX LP file, rows and variable names (x_m_i, y_m_i, z_m_i) as populatebyrow
 *                            creates them -- what cplex.exportModel writes to log/QPmodel_trajOpt.lp; HOST pointers, rows / sfc of
 *                            THIS instance ([n_obs*P] rows, [M] boxes); needs no device.
 *   lscqp_row_family_name    "SFC", "LSC", ... for messages. */
enum {
    LSCQP_ROW_BOUND = 0,         /* variable box = world box (:252-265) */
    LSCQP_ROW_SFC = 1,           /* corridor faces (:372-397) */
    LSCQP_ROW_LSC = 2,           /* LSC / BVC half-spaces (:399-437); obstacle = oi */
    LSCQP_ROW_VEL = 3,           /* :448-453 */
    LSCQP_ROW_ACC = 4,           /* :462-471 */
    LSCQP_ROW_COMM_PAIR = 5,     /* :480-489; obstacle = mi (the segment whose first point the row ties to) */
    LSCQP_ROW_COMM_WAYPOINT = 6, /* :492-498 */
    LSCQP_ROW_EQUALITY = 7,      /* initial state, joins, end stop (:318-368, 502-511) */
    LSCQP_ROW_FAMILIES = 8
};
typedef struct lscqp_diag { /* 128 bytes */
    double worst[LSCQP_ROW_FAMILIES];    /* largest violation per family (0 for a family without rows) */
    int32_t violated[LSCQP_ROW_FAMILIES]; /* rows violated by more than tol */
    double violation;                     /* of the most violated row overall ... */
    int32_t family, obstacle, segment, point, axis, reserved; /* ... and its name; -1 where a field does not apply */
} lscqp_diag;
int lscqp_diagnose_device(lscqp_handle h, int64_t n, const lscqp_header* d_hdr, const lscqp_row* d_rows, const uint64_t* d_row_offsets,
                          const lscqp_box* d_sfc, const double* d_x, double tol, lscqp_diag* d_out, void* stream);
int lscqp_diagnose(lscqp_handle h, int64_t n, const lscqp_header* hdr, const lscqp_row* rows, const uint64_t* row_offsets, const lscqp_box* sfc,
                   const double* x, double tol, lscqp_diag* out);
int lscqp_dump_instance(lscqp_handle h, const lscqp_header* hdr, const lscqp_row* rows, const lscqp_box* sfc, const char* path);
const char* lscqp_row_family_name(int32_t family);

/* ---- the PRESCREEN (round 14): per-control-point infeasibility, proven in one pass in front of the solve ----------------------
 *
 * The reference learns that a QP has no point from CPLEX's presolve and falls back at once (src/traj_optimizer.cpp:103-144: status
 * Infeasible / InfeasibleOrUnbounded -> QPFAILED; src/traj_planner.cpp:767-797: the caller keeps initial_traj).  The dual active-set phase
 * reaches the same verdict only after ~70 steps.  An LSC row (:413-429), a corridor face (:372-397) and a world face (:252-253) each touch
 * ONE control point: if the rows of one control point have no common point, the QP has none.  The prescreen (csrc/lscqp_prescreen.hip)
 * tests that per control point, one lane each: Goldfarb-Idnani in three variables on the point's LSC rows and its interval (world box,
 * corridor of its segment), and FIRES only with a certificate it has checked itself on the normalised rows n^_i.c >= b^_i, coordinates
 * relative to the agent's position p0:
 *     lambda >= 0, sum lambda = 1 over at most dim + 1 rows;  rho = sum lambda_i n^_i,  v = sum lambda_i b^_i;
 *     D = the largest distance from p0 to a corner of the world box (over the class's `dim` axes);
 *     violation = v - |rho|_1 D >= 1e-6 m  -- every point of the world box violates one of the rows by that much.
 * A control point whose rows are empty by 1e-5 m or more fires; one whose rows have a point to within 0.9e-6 m never does; in between either
 * answer is right.  Not tested: the fixed control points c0, c1, c2 of segment 0 (the reference puts no LSC row on them, :404-406), rows
 * that couple control points, RSFC classes, and an instance with n_obs < 0 or n_obs > n_obs_max.  One verdict per instance: the lowest
 * firing control point m*6 + i.
 *
 *   lscqp_prescreen_batch_device  the test alone: one certificate per instance, nothing else is written.  DEVICE pointers, asynchronous on
 *                            `stream`, capturable; arguments validated like lscqp_solve_batch_device's; LSCQP_ERR_NO_DEVICE without a device.
 *   lscqp_set_prescreen      LSCQP_PRESCREEN_OFF (default) / LSCQP_PRESCREEN_ON.  Waits for the device, and moves the handle's generation as
 *                            lscqp_update does: a plan drops its captured graph and re-captures.  lscqp_prescreen reads the mode back.
 * With the prescreen ON every solve entry that runs on one device (host-pointer, device, _ex, ordered, bound; through them lscqp_plan's
 * chain) enqueues the prescreen first on the same stream.  A fired instance gets what the phase's own INFEASIBLE verdict writes -- x_out =
 * the start (x_init, or hover at p0), obj 0, LSCQP_STATUS_INFEASIBLE, info {0, LSCQP_INFO_ACTIVE_SET | LSCQP_INFO_PRESCREENED, res_primal =
 * the proven violation, 0, 0} -- and every kernel behind skips it (the phase through a bit of its `behind` argument, the interior-point
 * passes by the ACTIVE_SET flag as for the phase's own verdict; as there, a caller that passes no info array leaves the later passes nothing to
 * recognise the verdict by, and they look at the instance again).  Every other instance is marked LSCQP_STATUS_ITER_LIMIT and solved exactly as
 * without the prescreen, bit for bit.  The one-launch fused form is not used while the prescreen is on (two launches, as with das_fused = 0);
 * with the phase off the first interior-point pass takes only what is marked ITER_LIMIT.  The sharded multi-device entries
 * call the device entry once per device and inherit the mode; nothing of theirs was changed for it.
 * OFF: nothing of this happens -- same launches, same arguments, same graph nodes. */
#define LSCQP_PRESCREEN_OFF 0
#define LSCQP_PRESCREEN_ON 1
#define LSCQP_INFO_PRESCREENED 128  /* lscqp_info.flags: LSCQP_STATUS_INFEASIBLE by the prescreen; res_primal = the proven violation */
typedef struct lscqp_prescreen_cert { /* 72 bytes */
    int32_t fired;         /* 0 / 1 */
    int32_t control_point; /* m*6 + i, -1 if not fired */
    int32_t n_rows;        /* 1..4, 0 if not fired */
    int32_t reserved;
    int32_t row[4];        /* >= 0: index into the instance's row list (oi * 6 M + control_point); -1-(2*axis+side): interval face, side 0 = lower */
    double lambda[4];      /* >= 0, sum 1 */
    double violation;      /* proven, metres (>= 1e-6 when fired) */
} lscqp_prescreen_cert;
int lscqp_prescreen_batch_device(lscqp_handle h, int64_t n, int32_t n_obs_max, const lscqp_header* d_hdr, const lscqp_row* d_rows,
                                 const uint64_t* d_row_offsets, const lscqp_box* d_sfc, lscqp_prescreen_cert* d_cert_out, void* stream);
int lscqp_set_prescreen(lscqp_handle h, int32_t mode);
int lscqp_prescreen(lscqp_handle h);

/* Number of inequality rows populatebyrow adds for an agent with n_obs obstacles (SFC + LSC + velocity +
 * acceleration + communication, src/traj_optimizer.cpp:370-500), not counting rows dropped for tiny normals. */
int lscqp_num_inequalities(lscqp_handle h, int32_t n_obs);

/* Algorithmic HBM bytes of one instance: rows + boxes + header in, x/obj/status out. */
int64_t lscqp_algorithmic_bytes(lscqp_handle h, int32_t n_obs);

/* Human-readable description of the last error on this thread. */
const char* lscqp_last_error(void);

/* "lscqp <major>.<minor> (gfx950, ...)" */
const char* lscqp_version(void);

#ifdef __cplusplus
}
#endif
#endif /* LSCQP_H */
