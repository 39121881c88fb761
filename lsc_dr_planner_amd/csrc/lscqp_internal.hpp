// lscqp_internal.hpp — the ONE declaration of every function the library's translation units call across each other (C linkage, not part
// of include/lscqp.h).  Every unit that defines or calls one of them includes this file: a definition that drifts from its declaration
// then fails to compile instead of linking and passing garbage.  api.py reads the prototypes of the entries its wrappers call
// (lscqp_optimize_goal_fin_device_, lscqp_commit_validate_raw_, lscqp_debug_*_) from this text.
// A public device entry is DEFINED in the unit that owns its kernel, checks in front of the launch; no `_raw_` half of it is declared here.
// The four `_raw_` functions that remain have a caller besides their own public entry: lscqp_generate_lsc_raw_ (four generator entries, the
// tests for M = 1), lscqp_generate_clsc_obstacles_raw_ (the tests for M = 1), lscqp_commit_validate_raw_ (lscplan.hip, api.py) and
// lscqp_map_raw_ (lscgrid.hip).
#ifndef LSCQP_INTERNAL_HPP
#define LSCQP_INTERNAL_HPP

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/lscqp.h"

namespace lscqp {
struct DevClass;  // lscqp_kernel.hpp; only ever behind a pointer here
}
namespace {
struct SolvePlan;  // lscqp_solve_plan.hpp (lscqp_api.hip alone completes it)
}

extern "C" {

// ---- lscqp_api.hip
int lscqp_set_error_(int code, const char* msg);
// for a device entry, after its argument checks: LSCQP_OK, or LSCQP_ERR_NO_DEVICE with the fixed text (there is no CPU fallback)
int lscqp_need_device_(void);
// ... and behind its launch: LSCQP_OK, or LSCQP_ERR_HIP with "HIP launch failed: <what the runtime says>"
int lscqp_launch_result_(hipError_t e);
const lscqp_class_desc* lscqp_class_desc_of_(lscqp_handle h);  // for lscplan.hip
uint64_t lscqp_handle_generation_(lscqp_handle h);
// (library-internal, lscqp_comm.hip) does a batch of this shape have a second chance on the instance with the other elimination order?
int lscqp_has_other_order_(lscqp_handle h, int64_t n, int32_t n_obs_max);
// (library-internal, tests and development tools) re-read the handle's switches from the environment / set one by name; -1 restores a
// launch-shape override to the policy's value
int lscqp_debug_reload_knobs_(lscqp_handle h);
int lscqp_debug_set_knob_(lscqp_handle h, const char* name, int value);
// (library-internal: every entry point that takes a mission partition) mission_offsets[0..n_missions], host: strictly increasing from 0 to n_total
int lscqp_check_missions_(int64_t n_total, int32_t n_missions, const int64_t* mission_offsets);
int lscqp_solve_batch_device_internal_(lscqp_handle h, int64_t n, int32_t n_obs_max, const lscqp_header* d_hdr, const lscqp_row* d_rows,
                                       const uint64_t* d_row_offsets, const lscqp_box* d_sfc, const double* d_x_init, double* d_x_out, double* d_obj_out,
                                       int32_t* d_status_out, lscqp_info* d_info_out, int32_t retry, int32_t part, const int32_t* d_order, void* stream,
                                       int* deferred);
// (library-internal, tests) the plan of a call of this handle, from the planner the worker above runs -- on no device: the CU count and
// whether the class's tables are on the device are arguments.  has_order: taken because a call has it; no rule reads it today.
int lscqp_debug_solve_plan_(lscqp_handle h, int64_t n, int32_t n_obs_max, int32_t retry, int32_t part, int32_t has_x_init, int32_t has_order,
                            int32_t deferred, int32_t n_cu, int32_t tables_available, SolvePlan* out);
// (library-internal, tests only) the prescreen's per-control-point arithmetic on HOST arrays (lscqp_prescreen.hip: lscqp_prescreen_host_twin_) -- holds the
// certificate contract to the referee on a machine without a device.  No entry point of the ABI calls it; the product path has no CPU fallback.
int lscqp_debug_prescreen_twin_(lscqp_handle h, int64_t n, int32_t n_obs_max, const lscqp_header* hdr, const lscqp_row* rows, const uint64_t* row_offsets,
                                const lscqp_box* sfc, lscqp_prescreen_cert* cert_out);

// ---- the generated lscqp_work_table.cpp (build.py; compiled by g++ without HIP, so it keeps its own definition and cannot include this file)
int lscqp_work_table_(int M, int D, int E, int S, int W, int X, double* out24);

// ---- lscqp_generic.hip: the run-time-shaped instance, every (M, dim, planner mode) / neighbour count the compiled table does not serve
int lscqp_generic_supports(int M, int dim, int es);
int lscqp_generic_max_obstacles(int M, int dim, int es);
size_t lscqp_generic_lds_bytes(int M, int dim, int es, int n_obs_max);
hipError_t lscqp_launch_generic(const lscqp::DevClass* cls, int M, int dim, int es, int64_t n, const lscqp_header* hdr, const lscqp_row* rows,
                                const uint64_t* row_offsets, const lscqp_box* sfc, const double* x_init, double* x_out, double* obj_out,
                                int32_t* status_out, lscqp_info* info_out, hipStream_t stream);

// ---- lscqp_das.hip: the dual active-set phase
size_t lscqp_das_build_tables(int M, int es, double dt, double w_c, double w_t, double* out);
size_t lscqp_das_build_pairs(int M, int dim, int comm_on, int32_t* out);
size_t lscqp_das_lds_bytes(int M, int dim, int kmax, int cacheC, int stage_rows);
int lscqp_das_blocks_per_cu(int M, int dim, int kmax, int rows_f32);
hipError_t lscqp_launch_das(const lscqp::DevClass* cls, int M, int dim, int es, int cap, int threads, int kmax, int max_steps, int cacheC,
                            int stage_rows, int screen, const double* d_tab, int64_t n, const lscqp_header* hdr, const lscqp_row* rows, const uint64_t* row_offsets,
                            const lscqp_box* sfc, const double* x_init, double* x_out, double* obj_out, int32_t* status_out,
                            lscqp_info* info_out, hipStream_t stream);

// ---- lscqp_prescreen.hip: cert_out for the standalone entry, the solve's outputs in front of a solve
hipError_t lscqp_launch_prescreen(const lscqp::DevClass* cls, int M, int dim, int cap, int64_t n, const lscqp_header* hdr, const lscqp_row* rows,
                                  const uint64_t* row_offsets, const lscqp_box* sfc, const double* x_init, lscqp_prescreen_cert* cert_out,
                                  double* x_out, double* obj_out, int32_t* status_out, lscqp_info* info_out, hipStream_t stream);
// (library-internal, tests only) test_point over a batch in HOST memory, control point by control point in index order: the kernel's own
// arithmetic without a device, so that the certificate contract can be held to the referee where no GPU is.  No entry point of the ABI calls it.
int lscqp_prescreen_host_twin_(const lscqp::DevClass* cls, int M, int dim, int cap, int64_t n, const lscqp_header* hdr, const void* rows,
                               const uint64_t* row_offsets, const lscqp_box* sfc, lscqp_prescreen_cert* cert_out);

// ---- lscgen.hip
// (library-internal: the generator entries, and the tests for M = 1) one launch of the generator, no checks
int lscqp_generate_lsc_raw_(int mode, int M, int dim, int64_t n_agents, int32_t n_obs, int64_t first_agent,
                            const double* d_traj, const double* d_own_traj, const int32_t* d_neighbours, const double* d_radius,
                            const double* d_downwash, const double* d_goal, const double* d_goal_all, int rows_f32,
                            int32_t n_obs_total, int32_t slot0, lscqp_row* d_rows_out, void* stream);
// (library-internal: lscqp_generate_obstacle_rows_device, and the tests for M = 1) one launch of generateCLSC's non-agent rows, no checks
int lscqp_generate_clsc_obstacles_raw_(int M, int dim, double dt, double obs_downwash_threshold, int64_t n_agents, int32_t n_dyn,
                                       int64_t first_agent, const double* d_traj, const int32_t* d_obstacle_ids,
                                       const lscqp_obstacle* d_obstacles, const double* d_obstacle_goal, const double* d_radius,
                                       const double* d_goal, int rows_f32, int32_t n_obs_total, int32_t slot0, lscqp_row* d_rows_out,
                                       void* stream);
// (library-internal, lscplan.hip) lscqp_generate_constraints_device_ex with the planning agents' initial trajectories kept apart from
// the predicted trajectories of the agents as obstacles: d_own_traj [n_agents][M][6][3], NULL = rows d_traj[first_agent + a]
int lscqp_generate_constraints_own_(lscqp_handle h, int32_t mode, int64_t n_agents, int32_t n_obs, int64_t first_agent,
                                    const double* d_traj, const double* d_own_traj, const int32_t* d_neighbours, const double* d_radius,
                                    const double* d_downwash, const double* d_goal_all, lscqp_row* d_rows_out, int32_t n_obs_total,
                                    int32_t slot0, void* stream);

// ---- lscgoal.hip
// (library-internal, lscplan.hip) the goal LP that also finishes the headers of the chain: goal as a point3d, terminal_segments (fin_dt = the class's dt)
int lscqp_optimize_goal_fin_device_(lscqp_handle h, int64_t n, lscqp_header* d_hdr, const lscqp_row* d_rows, const uint64_t* d_row_offsets,
                                    const lscqp_box* d_sfc, int32_t* d_status_out, double fin_dt, void* stream);

// ---- lscpost.hip
// (library-internal, lscplan.hip) commit + isSolValid + doStep of the local agents in one launch; d_x_plan / d_goal: the local block
int lscqp_commit_validate_raw_(int M, int dim, int use_sfc, double dt, int64_t n, double time_step, double z_2d, const int32_t* d_qp_status,
                               const double* d_x_new, const double* d_x_init, double* d_x_plan, double* d_goal, const lscqp_header* d_hdr,
                               const lscqp_box* d_sfc, int32_t* d_valid, double* d_state, void* stream);

// ---- lscsfc.hip, lscsfc_tp.hip
int lscqp_map_device_(lscqp_map mp);
uint64_t lscqp_map_generation_(lscqp_map mp);
// (library-internal: lscgrid.hip evaluates the grid planner's occupancy from the same nearest-occupied-cell field)
int lscqp_map_raw_(lscqp_map mp, double* res, float* world_min, float* world_max, int* key0, int* dims, const int32_t** d_nearest, int* device);
hipError_t lscsfc_launch_throughput_(const void* view, int mode, int M, int64_t n, const double* d_points, const double* d_radius,
                                     lscqp_box* d_sfc, int32_t* d_status_out, void* stream);  // lscsfc_tp.hip
hipError_t lscsfc_launch_throughput_worlds_(const void* view, int mode, int M, int64_t n, const double* d_points, const double* d_radius,
                                            lscqp_box* d_sfc, int32_t* d_status_out, const void* d_table, const int32_t* d_world_of, void* stream);
int lscsfc_throughput_max_cells_(void);
// (library-internal: lscgrid.hip, lscplan.hip) a set of worlds: its members, the sum of their generation counters (it only rises), its
// table rewritten if a member was prepared behind its back (waits for the device), and the first field in which the set's shape or device
// differs from a map's (NULL: none)
int lscqp_worlds_count_(lscqp_worlds w);
lscqp_map lscqp_worlds_map_(lscqp_worlds w, int k);
uint64_t lscqp_worlds_generation_(lscqp_worlds w);
int lscqp_worlds_refresh_(lscqp_worlds w);
const char* lscqp_worlds_shape_difference_(lscqp_worlds w, lscqp_map mp);

// ---- lscgrid.hip
// (library-internal, also lscplan.hip) work arrays for n agents in n_missions missions; grows on demand, which synchronises and allocates
int lscqp_grid_reserve_missions_(lscqp_grid g, int64_t n, int32_t n_missions);

// ---- lscrecord.hip
// (library-internal, lscplan.hip) d_offsets_borrowed: the partition's offsets as the plan already has them on the device; NULL: an own copy
int lscqp_record_create_(lscqp_handle h, int64_t n_total, int32_t n_missions, const int64_t* mission_offsets,
                         const int64_t* d_offsets_borrowed, int32_t n_samples, double record_time_step, double time_step, double z_2d,
                         const lscqp_record_desc* desc, lscqp_record* out);
// (library-internal, lscplan.hip: lscqp_plan_run) the unfinished word as `stream` leaves it, waited for
int lscqp_record_unfinished_on_(lscqp_record r, void* stream, int32_t* unfinished_out);

// ---- lscplan.hip
const lscqp_plan_desc* lscqp_plan_desc_of_(lscqp_plan p);  // (library-internal: lscqp_comm.hip)
int lscqp_plan_device_(lscqp_plan p);

// ---- lscqp_diag.hip
int lscqp_debug_calibrate_(int64_t bytes, void* stream);

}  // extern "C"

#endif  // LSCQP_INTERNAL_HPP
