// lscgrid.hip — the grid planner / MAPF layer of the reference on the device, gfx950 only: where each agent's NEXT WAYPOINT comes from.
//   GridBasedPlanner::updateGridInfo / updateGridMap / updateGridMission   reference src/grid_based_planner.cpp:86-140, 255-283
//   Grid::Grid (x-y, 4-connected: left, right, up, down)                    third_party/grid-pathfinding/graph/src/graph.cpp:371-400
//   Solver::createDistanceTable                                             src/mapf/solver.cpp:270-289
//   PIBT::run / funcPIBT / planOneStep / chooseNode, FIRST timestep only    src/mapf/pibt.cpp
//   MultiSyncSimulator::decentralizedMAPP (groups, update filter)           src/multi_sync_simulator.cpp:160-303
// Three pieces:
//   occupancy   one lane per grid node, from the voxel map's nearest-occupied-cell field (the corridor kernel's own query, quirk included)
//   fields      one workgroup per agent: the distance-to-goal field of the agent relaxed in sweeps -- d = min(d, min over the 4 neighbours + 1)
//               until a sweep changes nothing (a workgroup-wide vote) -- in LDS where the field fits, in its place in HBM otherwise
//   waypoints   one replan's decision: candidates gathered by all lanes, then ONE workgroup: groups by min-label propagation, agents ordered by
//               priority, the PIBT walk (sequential by nature: priority inheritance and backtracking) by one wavefront with an explicit
//               stack, and the simulator's update filter by all lanes again.  A second, WIDE form spreads the same decision over the device
//               (below).  The two forms share ONE walk (pibt_walk, over a dense or a keyed node table), ONE set of filter tests
//               (filter_abc), ONE fixed point (find_valid_update) and ONE waypoint write (write_update); what differs stays in the kernels:
//               how occupied_now is seeded, how the tables are cleared, and what the pass bound counts
// A MISSION PARTITION (include/lscqp.h, "many missions over one map") cuts the agents into contiguous slices that share the map and nothing
// else: one occupancy copy per mission (start and goal nodes are cleared in the agent's own copy only), and the decision as one workgroup per
// mission over its slice, with node tables, order, stack, fail flag and walk bound of its own.
// Everything here is integers and exact grid points, and the float32 / double arithmetic of the reference where a comparison is made.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/lscqp.h"
#include "lscqp_device.hpp"
#include "lscqp_missions.hpp"
#include "lscqp_internal.hpp"


namespace lscgrid {

using lscqp_missions::mission_of;
constexpr int kUnreach = LSCQP_GRID_UNREACHABLE;
constexpr int kBlocked = kUnreach + 1;    // an occupied node while a field is relaxed in HBM (written out as kUnreach)
constexpr unsigned kUnreach16 = 0xFFFEu;  // the same pair where the field is relaxed in LDS (16 bits per node)
constexpr unsigned kBlocked16 = 0xFFFFu;
constexpr int kLdsNodes = 65000;          // padded nodes a 16-bit LDS field holds: paths stay below kUnreach16, 130 KB of the CU's 160 KB
constexpr double kEpsFloat = 1e-5;        // SP_EPSILON_FLOAT
constexpr int kDecideThreads = 1024;
constexpr int kTableLdsBytes = 60 * 1024;  // occupied_now / occupied_next live in LDS up to this size, in HBM beyond

struct View {  // the grid as the kernels see it
    double gmin0, gmin1, res, z_2d;
    int W, H;
};

struct MapRaw {
    double res;
    int key00, key01, key02, dims0, dims1, dims2;
    const int32_t* nearest;
};

// gridNodeToPoint3D (:386-399): grid_min + index * resolution in double, held as point3d (float32)
__device__ __forceinline__ float node_coord(double gmin, int i, double res) {
#pragma clang fp contract(off)
    return (float)(gmin + (double)i * res);
}

// point3DToGridVector (:429-441): round((point - grid_min) / resolution), clamped into the grid
__device__ __forceinline__ int coord_node(float p, double gmin, double res, int dim) {
#pragma clang fp contract(off)
    int v = (int)round(((double)p - gmin) / res);
    return v < 0 ? 0 : (v > dim - 1 ? dim - 1 : v);
}

__device__ __forceinline__ int point_node(const View& g, const double* p) {
    return coord_node((float)p[1], g.gmin1, g.res, g.H) * g.W + coord_node((float)p[0], g.gmin0, g.res, g.W);
}

// updateGridMap (:102-140): a node is occupied when the L-infinity distance from it to the nearest occupied voxel CELL is below
// agent_radius - SP_EPSILON_FLOAT.  The query is the corridor kernel's (lscsfc.hip obstacle_in): no cell within max_dist, or a node outside the
// distance map, leaves the reference's closest_point default-constructed -- a cell at the world origin.
__global__ __launch_bounds__(256) void occupancy_kernel(View g, MapRaw m, double radius, uint8_t* __restrict__ occ) {
#pragma clang fp contract(off)
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= g.W * g.H) return;
    const int j = id / g.W, i = id - j * g.W;
    const float p[3] = {node_coord(g.gmin0, i, g.res), node_coord(g.gmin1, j, g.res), (float)g.z_2d};
    const int key0[3] = {m.key00, m.key01, m.key02}, dims[3] = {m.dims0, m.dims1, m.dims2};
    int v[3];
    bool inside = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        v[k] = (int)floor((1.0 / m.res) * (double)p[k]) - key0[k];
        inside = inside && v[k] >= 0 && v[k] < dims[k];
    }
    const int code = inside ? m.nearest[((int64_t)v[2] * dims[1] + v[1]) * dims[0] + v[0]] : 0;
    const bool have = (code >> 24) != 0;
    const int off[3] = {(code & 255) - 128, ((code >> 8) & 255) - 128, ((code >> 16) & 255) - 128};
    const float delta = (float)(0.5 * m.res);
    double dist = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float c = have ? (float)(((double)(v[k] + off[k] + key0[k]) + 0.5) * m.res) : 0.0f;
        const float cmin = c - delta, cmax = c + delta;
        const float q = p[k] < cmin ? cmin : (p[k] > cmax ? cmax : p[k]);
        const double dk = fabs((double)(q - p[k]));
        dist = dist < dk ? dk : dist;
    }
    occ[id] = dist < radius - kEpsFloat ? 1 : 0;
}

// one copy of the base occupancy per mission
__global__ __launch_bounds__(256) void spread_occupancy_kernel(int nodes, int K, const uint8_t* __restrict__ base, uint8_t* __restrict__ copies) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (int64_t)nodes * K) return;
    copies[id] = base[id % nodes];
}

// updateGridMission (:255-283), once per mission instead of once per group and replan (include/lscqp.h): start and goal nodes are free.
// off != NULL: occ holds one copy per mission of the partition and an agent clears its nodes in the copy of its own mission only
__global__ __launch_bounds__(256) void clear_nodes_kernel(View g, int64_t n, const double* __restrict__ start, const double* __restrict__ goal,
                                                          uint8_t* occ, const int64_t* __restrict__ off, int K) {
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= n) return;
    if (off) occ += (int64_t)mission_of(off, K, a) * g.W * g.H;
    occ[point_node(g, start + a * 3)] = 0;
    occ[point_node(g, goal + a * 3)] = 0;
}

// createDistanceTable as a relaxation.  One workgroup per agent.  LDS form: the field carries a border of blocked nodes, so a node's four
// neighbours are at -1, +1, -pitch, +pitch with no bounds to test; HBM form: the same sweeps over the agent's slice of `field` itself.
// Lanes read their neighbours while other lanes lower them: every value ever stored is the length of SOME path to the goal, values only
// fall, and a sweep in which nothing changed saw constant values -- the fixed point, which is the BFS distance.
template <bool LDS>
__global__ __launch_bounds__(1024) void fields_kernel(View g, const uint8_t* __restrict__ occ, const double* __restrict__ start,
                                                      const double* __restrict__ goal, int32_t* field, int32_t* __restrict__ init_d,
                                                      const int64_t* __restrict__ off, int K) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int64_t a = blockIdx.x;
    const int T = blockDim.x, tid = threadIdx.x, W = g.W, H = g.H, nodes = W * H;
    if (off) occ += (int64_t)mission_of(off, K, a) * nodes;  // (the copy of the agent's mission)
    const int gnode = point_node(g, goal + a * 3), snode = point_node(g, start + a * 3);
    int32_t* out = field + a * (int64_t)nodes;
    if (LDS) {
        uint16_t* f = (uint16_t*)smem;
        const int P = W + 2, padded = P * (H + 2);
        for (int id = tid; id < padded; id += T) f[id] = (uint16_t)kBlocked16;
        __syncthreads();
        for (int id = tid; id < nodes; id += T) {
            const int y = id / W, x = id - y * W;
            f[(y + 1) * P + x + 1] = (uint16_t)(id == gnode ? 0u : (occ[id] ? kBlocked16 : kUnreach16));
        }
        __syncthreads();
        for (int sweep = 0; sweep <= nodes; sweep++) {  // (a path has fewer than `nodes` edges: the vote ends the loop long before)
            int changed = 0;
            for (int id = P + 1 + tid; id < padded - P - 1; id += T) {
                const unsigned d = f[id];
                if (d == kBlocked16 || d == 0u) continue;
                const unsigned l = f[id - 1], r = f[id + 1], u = f[id - P], dn = f[id + P];
                const unsigned m = min(min(l, r), min(u, dn)) + 1u;
                if (m < d) {
                    f[id] = (uint16_t)m;
                    changed = 1;
                }
            }
            if (!__syncthreads_or(changed)) break;
        }
        for (int id = tid; id < nodes; id += T) {
            const int y = id / W, x = id - y * W;
            const unsigned d = f[(y + 1) * P + x + 1];
            out[id] = d >= kUnreach16 ? kUnreach : (int)d;
        }
        if (tid == 0) {
            const int y = snode / W, x = snode - y * W;
            const unsigned d = f[(y + 1) * P + x + 1];
            init_d[a] = d >= kUnreach16 ? kUnreach : (int)d;
        }
    } else {
        for (int id = tid; id < nodes; id += T) out[id] = id == gnode ? 0 : (occ[id] ? kBlocked : kUnreach);
        __syncthreads();
        for (int sweep = 0; sweep <= nodes; sweep++) {
            int changed = 0;
            for (int id = tid; id < nodes; id += T) {
                const int d = out[id];
                if (d == kBlocked || d == 0) continue;
                const int y = id / W, x = id - y * W;
                int m = kBlocked;
                if (x > 0) m = min(m, out[id - 1]);
                if (x + 1 < W) m = min(m, out[id + 1]);
                if (y > 0) m = min(m, out[id - W]);
                if (y + 1 < H) m = min(m, out[id + W]);
                if (m + 1 < d) {
                    out[id] = m + 1;
                    changed = 1;
                }
            }
            if (!__syncthreads_or(changed)) break;
        }
        for (int id = tid; id < nodes; id += T)
            if (out[id] == kBlocked) out[id] = kUnreach;
        __syncthreads();
        if (tid == 0) init_d[a] = out[snode];
    }
}

// ---- one replan's waypoint decision --------------------------------------------------------------------------------------------------------
struct Scratch {  // per-agent work arrays of a decision (lscqp_grid_reserve) and the two node tables of the HBM form
    int32_t *cur, *cand, *cost, *vnext, *order, *stack, *label, *blocker, *keep, *onnode, *gsize;
    int32_t *now, *next;  // [nodes] each, all zero between launches
    int32_t* status;
};

// Words the ONE workgroup of the decision kernel changes while other lanes read them: relaxed atomics at workgroup scope -- plain loads and
// stores to the hardware (a workgroup's wavefronts share their CU's L1), but never kept in a register by the compiler
__device__ __forceinline__ int ldv(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void stv(int32_t* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// every lane: an agent's PIBT node (the node of its present WAYPOINT, multi_sync_simulator.cpp:205), its five candidates in the identity
// order left, right, up, down, stay with their distances to the agent's goal, and the start of the group labels
// MIS: the agents are partitioned into missions off[0..K]; occ holds one copy per mission and the labels are local to the mission's slice
template <bool MIS>
__global__ __launch_bounds__(256) void gather_kernel(View g, int64_t n, double range, const uint8_t* __restrict__ occ,
                                                     const double* __restrict__ waypoint, const int32_t* __restrict__ field, Scratch s,
                                                     const int64_t* __restrict__ off, int K) {
#pragma clang fp contract(off)
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= n) return;
    const int W = g.W, H = g.H;
    int64_t base = 0;
    if (MIS) {
        const int k = mission_of(off, K, a);
        base = off[k];
        occ += (int64_t)k * W * H;
    }
    const float wx = (float)waypoint[a * 3 + 0], wy = (float)waypoint[a * 3 + 1], wz = (float)waypoint[a * 3 + 2];
    const int cx = coord_node(wx, g.gmin0, g.res, W), cy = coord_node(wy, g.gmin1, g.res, H);
    const int cur = cy * W + cx;
    const float dx = wx - node_coord(g.gmin0, cx, g.res), dy = wy - node_coord(g.gmin1, cy, g.res), dz = wz - (float)g.z_2d;
    s.onnode[a] = sqrt((double)(dx * dx + dy * dy + dz * dz)) < kEpsFloat ? 1 : 0;  // (the waypoint IS its node's point, to Vector3::distance)
    s.cur[a] = cur;
    const int32_t* f = field + a * (int64_t)W * H;
    const int ox[5] = {-1, 1, 0, 0, 0}, oy[5] = {0, 0, -1, 1, 0};
#pragma unroll
    for (int c = 0; c < 5; c++) {
        const int x = cx + ox[c], y = cy + oy[c];
        int u = -1;
        if (x >= 0 && x < W && y >= 0 && y < H) {
            u = y * W + x;
            if (c < 4 && occ[u]) u = -1;  // (the agent's own node is a node of its graph whatever the map says)
        }
        s.cand[a * 5 + c] = u;
        s.cost[a * 5 + c] = u >= 0 ? f[u] : kUnreach;
    }
    s.vnext[a] = -1;
    s.blocker[a] = -1;
    s.gsize[a] = 0;
    s.label[a] = range < 0 ? 0 : (int)(a - base);
}

// PIBT::chooseNode for an agent nobody else can see (a group of one): the goal if it is a candidate, else the first candidate of the least
// distance (the stay node is the only one occupied now and the last one visited, so the occupied-now tie rule never fires)
__device__ __forceinline__ int choose_alone(const Scratch& s, int64_t a) {
    int v = -1, cv = 0;
    for (int c = 0; c < 5; c++) {
        const int u = s.cand[a * 5 + c], cu = s.cost[a * 5 + c];
        if (u < 0) continue;
        if (cu == 0) return u;
        if (v < 0 || cu < cv) v = u, cv = cu;
    }
    return v;
}

// ---- what the two forms of the decision share: the walk of one group, the update filter, the waypoint write ----------------------------------
// occupied_now / occupied_next behind a slot index.  Dense: slot = node, every node has a slot (the one-workgroup form: LDS or the HBM slab)
struct DenseTables {
    int32_t *now, *next;
    __device__ __forceinline__ int find(int node) const { return node; }
    __device__ __forceinline__ int claim(int node) const { return node; }
};

__device__ __forceinline__ unsigned table_hash(int node, unsigned mask) { return ((unsigned)node * 2654435761u >> 7) & mask; }

// Keyed: a group's own open-addressed table of mask + 1 slots (the wide form); a node without a slot reads as 0 in both tables
struct KeyedTables {
    int32_t *tkey, *now, *next;
    unsigned mask;
    __device__ __forceinline__ int find(int node) const {  // the slot of `node`, -1 where the table has none
        for (unsigned h = table_hash(node, mask), probes = 0; probes <= mask; h = (h + 1) & mask, probes++) {
            const int k = ldv(tkey + h);
            if (k == node) return (int)h;
            if (k < 0) return -1;
        }
        return -1;
    }
    __device__ __forceinline__ int claim(int node) const {  // find or insert, by every lane of the walking wavefront alike; -1: the table is full
        for (unsigned h = table_hash(node, mask), probes = 0; probes <= mask; h = (h + 1) & mask, probes++) {
            const int k = ldv(tkey + h);
            if (k == node || k < 0) {
                if (k < 0) stv(tkey + h, node);
                return (int)h;
            }
        }
        return -1;
    }
};

// PIBT::run's planning loop for the first timestep over the members order[0..count) of ONE group, by ONE wavefront; occupied_now is seeded
// by the caller.  Every lane runs the same control flow and issues the same stores (a lane then reads back what it wrote itself); lanes 0..4
// look at one candidate each in chooseNode.  funcPIBT is entered at most once per agent and every entry plans once, plus once more after each
// child that failed (a child fails at most once): <= 2 n plans and <= n returns that carry "true" upwards -- 3 n passes of the loop below.
// `passes` counts them against `bound`, both the caller's; returns 1 where the bound was reached (the tables were corrupt), 0 otherwise.
template <class Tables>
__device__ __forceinline__ int pibt_walk(const Scratch& s, const Tables& t, const int32_t* order, int count, int32_t* stack, int lane, int& passes,
                                         int bound) {
    for (int idx = 0; idx < count; idx++) {
        const int a0 = ldv(order + idx);
        if (ldv(s.vnext + a0) != -1) continue;
        int sp = 0, mode = 0;  // mode 0: call or "the child failed" (plan a step), 1: the callee returned true
        stv(stack, a0);
        while (sp >= 0) {
            if (++passes > bound) return 1;
            if (mode == 1) {
                sp--;
                continue;
            }
            const int ai = ldv(stack + sp), cur_i = s.cur[ai];
            // chooseNode, candidates in the identity order (one of the orders std::shuffle can draw)
            int u = -1, cu = 0, held = 0, ok = 0, aj = -1;
            if (lane < 5) {
                u = s.cand[(int64_t)ai * 5 + lane];
                cu = s.cost[(int64_t)ai * 5 + lane];
                if (u >= 0) {
                    const int sl = t.find(u);
                    aj = sl >= 0 ? ldv(t.now + sl) - 1 : -1;
                    held = aj >= 0;
                    ok = sl < 0 || ldv(t.next + sl) == 0;              // vertex conflict
                    if (ok && aj >= 0) ok = ldv(s.vnext + aj) != cur_i;  // swap conflict
                }
            }
            int v = -1, cv = 0, hv = 0, jv = -1;
            for (int c = 0; c < 5; c++) {
                const int uc = __shfl(u, c), cc = __shfl(cu, c), hc = __shfl(held, c), oc = __shfl(ok, c), jc = __shfl(aj, c);
                if (!oc) continue;
                if (cc == 0) {  // the goal: taken at once
                    v = uc, jv = jc;
                    break;
                }
                if (v < 0 || cc < cv || (cc == cv && hv && !hc)) v = uc, cv = cc, hv = hc, jv = jc;
            }
            const int take = v < 0 ? cur_i : v;  // (failed to secure a node: stay, and tell the caller)
            const int sl = t.claim(take);
            if (sl < 0) return 1;  // (never: a dense table has every node, a keyed one is at most half full)
            stv(t.next + sl, ai + 1);
            stv(s.vnext + ai, take);
            if (v < 0) {
                stv(s.blocker + ai, -1);
                sp--;
                mode = 0;
                continue;
            }
            stv(s.blocker + ai, (jv != ai && v != cur_i) ? jv : -1);
            if (jv >= 0 && jv != ai && ldv(s.vnext + jv) == -1) {  // priority inheritance
                sp++;
                if (sp >= count) return 1;  // (never: an agent is entered once)
                stv(stack + sp, jv);
                mode = 0;
                continue;
            }
            sp--;
            mode = 1;
        }
    }
    return 0;
}

// the update filter (:222-264) for one agent whose desired node is d: (a) the desired waypoint within range / 2 of every segment start and of
// the last point of the agent's plan, (b) it differs from the present waypoint, (c) the current goal point has reached the present waypoint
__device__ __forceinline__ int filter_abc(const View& g, double range, int M, int dim, const double* __restrict__ state, const double* __restrict__ plan,
                                          const double* __restrict__ cur_goal, const double* waypoint, int64_t a, int d) {
#pragma clang fp contract(off)
    const float zf = (float)g.z_2d;
    const int dy_ = d / g.W, dx_ = d - dy_ * g.W;
    const float des[3] = {node_coord(g.gmin0, dx_, g.res), node_coord(g.gmin1, dy_, g.res), zf};
    bool in_range = true;
    if (range > 0) {
        for (int m = 0; m <= M && in_range; m++) {
            double dist = 0;
            for (int k = 0; k < 3; k++) {
                float q;
                if (plan == nullptr) q = (float)state[a * 9 + k];
                else if (k >= dim) q = zf;
                else q = (float)plan[a * dim * M * 6 + ((int64_t)k * M + (m < M ? m : M - 1)) * 6 + (m < M ? 0 : 5)];
                const double dk = fabs((double)(des[k] - q));
                dist = dist < dk ? dk : dist;
            }
            if (dist > 0.5 * range - kEpsFloat) in_range = false;
        }
    }
    float nw = 0, ng = 0;
    for (int k = 0; k < 3; k++) {
        const float wv = (float)waypoint[a * 3 + k], e = des[k] - wv, h = (float)cur_goal[a * 3 + k] - wv;
        nw += e * e;
        ng += h * h;
    }
    return (in_range && sqrt((double)nw) > kEpsFloat && sqrt((double)ng) < kEpsFloat) ? 1 : 0;
}

// (d) "find valid update" (:266-296) by every lane of the workgroup, over the members order[0..count) or, order == nullptr, the agents
// 0..count: a candidate whose desired node is the present waypoint of a group member that is not (or no longer) a candidate itself is
// dropped, until nothing is.  Within a group PIBT hands out distinct nodes, so the only agent that can hold a candidate's desired node is
// the one PIBT found there -- `blocker`, a member of the same group -- and dropping candidates only ever adds holders: the loop's result
// does not depend on the order in which the reference visits its std::set.
template <int T>  // (the workgroup's size)
__device__ __forceinline__ void find_valid_update(const Scratch& s, const int32_t* order, int count) {
    for (int round = 0; round <= count; round++) {
        int changed = 0;
        for (int i = threadIdx.x; i < count; i += T) {
            const int a = order ? order[i] : i;
            if (!ldv(s.keep + a)) continue;
            const int j = ldv(s.blocker + a);
            if (j >= 0 && s.onnode[j] && !ldv(s.keep + j)) {
                stv(s.keep + a, 0);
                changed = 1;
            }
        }
        if (!__syncthreads_or(changed)) break;
    }
}

// an agent's verdict: where it updates, its waypoint becomes the desired node's grid point -- float32, as the reference holds it
__device__ __forceinline__ void write_update(const View& g, int up, int d, double* waypoint, int32_t* updated) {
#pragma clang fp contract(off)
    if (up) {
        const int dy_ = d / g.W, dx_ = d - dy_ * g.W;
        waypoint[0] = (double)node_coord(g.gmin0, dx_, g.res);
        waypoint[1] = (double)node_coord(g.gmin1, dy_, g.res);
        waypoint[2] = (double)(float)g.z_2d;
    }
    *updated = up;
}

// MIS: one workgroup per mission of the partition off[0..gridDim.x].  The workgroup sees its slice as a swarm of its own: every per-agent
// array is entered at the slice's first agent and agent ids are LOCAL to the slice from here on (labels, order, stack, the ids in the node
// tables; tie_breaker = id / n orders a contiguous slice the same either way), the node tables are the workgroup's own (LDS, or the
// mission's slab of the HBM tables) and so are the fail flag, the walk bound and the status word.  Only group_out speaks global ids.
template <bool MIS>
__global__ __launch_bounds__(kDecideThreads) void decide_kernel(View g, int64_t n64, double range, int M, int dim, int tables_in_lds,
                                                                const double* __restrict__ state, const double* __restrict__ plan,
                                                                const double* __restrict__ cur_goal, const int32_t* __restrict__ init_d,
                                                                double* waypoint, Scratch s, int32_t* __restrict__ group_out,
                                                                int32_t* __restrict__ desired_out, int32_t* __restrict__ updated_out,
                                                                const int64_t* __restrict__ off) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int n_multi_sh, fail_sh;
    int64_t base = 0;
    if (MIS) {
        const int64_t k = blockIdx.x;
        base = off[k];
        n64 = off[k + 1] - base;
        state += base * 9, cur_goal += base * 3, init_d += base, waypoint += base * 3;
        if (plan != nullptr) plan += base * dim * M * 6;
        group_out += base, desired_out += base, updated_out += base;
        s.cur += base, s.vnext += base, s.order += base, s.stack += base, s.label += base, s.blocker += base, s.keep += base, s.onnode += base;
        s.gsize += base, s.cand += base * 5, s.cost += base * 5;
        s.now += k * 2 * (int64_t)g.W * g.H, s.next += k * 2 * (int64_t)g.W * g.H;
        s.status += k;
    }
    const int n = (int)n64, tid = threadIdx.x, T = kDecideThreads, nodes = g.W * g.H;
    int32_t *now = s.now, *next = s.next;
    if (tables_in_lds) {
        now = (int32_t*)smem;
        next = now + nodes;
        for (int id = tid; id < 2 * nodes; id += T) now[id] = 0;
    }
    if (tid == 0) n_multi_sh = 0, fail_sh = 0;
    __syncthreads();
    // -- groups (decentralizedMAPP :162-193): connected components of "L-infinity distance of the current POSITIONS < range", as the least id of
    // the component.  Every label ever stored is the id of a member of the agent's own component and labels only fall, so reading them while other
    // lanes lower them (and jumping label -> label[label]) is safe; a round in which nothing changed is the fixed point.
    if (range > 0) {  // (range 0: nobody is within it, every agent keeps its own label)
        for (int round = 0; round <= n; round++) {
            int changed = 0;
            for (int a = tid; a < n; a += T) {
                const float px = (float)state[(int64_t)a * 9], py = (float)state[(int64_t)a * 9 + 1], pz = (float)state[(int64_t)a * 9 + 2];
                const int la = ldv(s.label + a);
                int m = la;
                for (int j = 0; j < n; j++) {
                    const int lj = ldv(s.label + j);
                    if (lj >= m) continue;
                    const double d0 = fabs((double)(px - (float)state[(int64_t)j * 9])), d1 = fabs((double)(py - (float)state[(int64_t)j * 9 + 1])),
                                 d2 = fabs((double)(pz - (float)state[(int64_t)j * 9 + 2]));
                    if (fmax(d0, fmax(d1, d2)) < range) m = lj;
                }
                const int mm = ldv(s.label + m);
                if (mm < m) m = mm;
                if (m < la) {
                    stv(s.label + a, m);
                    changed = 1;
                }
            }
            if (!__syncthreads_or(changed)) break;
        }
    }
    for (int a = tid; a < n; a += T) atomicAdd(s.gsize + ldv(s.label + a), 1);
    __syncthreads();
    // -- agents of a group of one decide by themselves; the others are ordered: group by group, within a group by PIBT's priority (elapsed is 0 at
    // the first timestep; larger init_d first, then the larger tie_breaker = id / n)
    for (int a = tid; a < n; a += T) {
        const int la = ldv(s.label + a);
        if (ldv(s.gsize + la) == 1) {
            const int v = choose_alone(s, a);
            stv(s.vnext + a, v < 0 ? s.cur[a] : v);
            continue;
        }
        atomicAdd(&n_multi_sh, 1);
        const int da = init_d[a];
        int rank = 0;
        for (int b = 0; b < n; b++) {
            const int lb = ldv(s.label + b);
            if (b == a || ldv(s.gsize + lb) == 1) continue;
            const int db = init_d[b];
            const bool before = lb != la ? lb < la : (db != da ? db > da : b > a);
            rank += before ? 1 : 0;
        }
        stv(s.order + rank, a);
    }
    __syncthreads();
    const int n_multi = n_multi_sh;
    // -- PIBT::run's planning loop for the first timestep, one group after the other, by ONE wavefront (pibt_walk).  The passes of all groups
    // count against ONE bound, 4 n + 16; reaching it means the tables were corrupt: the waypoints are then left alone and the status word says so.
    if (tid < 64) {
        const int lane = tid;
        const DenseTables t{now, next};
        const int bound = 4 * n + 16;
        int passes = 0, fail = 0;
        for (int gs = 0; gs < n_multi && !fail;) {
            const int ge = gs + ldv(s.gsize + ldv(s.label + ldv(s.order + gs)));
            for (int idx = gs + lane; idx < ge; idx += 64) {  // occupied_now: the last id wins
                const int a = ldv(s.order + idx);
                atomicMax(now + s.cur[a], a + 1);
            }
            __threadfence_block();
            __builtin_amdgcn_wave_barrier();
            fail = pibt_walk(s, t, s.order + gs, ge - gs, s.stack, lane, passes, bound);
            __threadfence_block();
            __builtin_amdgcn_wave_barrier();
            for (int idx = gs + lane; idx < ge; idx += 64) {  // leave the tables empty for the next group
                const int a = ldv(s.order + idx), vn = ldv(s.vnext + a);
                stv(now + s.cur[a], 0);
                if (vn >= 0) stv(next + vn, 0);
            }
            __threadfence_block();
            __builtin_amdgcn_wave_barrier();
            gs = ge;
        }
        if (fail) {
            if (!tables_in_lds)
                for (int id = lane; id < 2 * nodes; id += 64) stv(id < nodes ? now + id : next + (id - nodes), 0);
            if (lane == 0) fail_sh = 1;
        }
    }
    __syncthreads();
    const int fail = fail_sh;
    // -- the update filter: tests (a)-(c) per agent, then "find valid update" over the whole swarm (a blocker is a member of the agent's own group)
    for (int a = tid; a < n; a += T) {
        const int vn = ldv(s.vnext + a), d = vn < 0 ? s.cur[a] : vn;
        stv(s.keep + a, filter_abc(g, range, M, dim, state, plan, cur_goal, waypoint, a, d));
        desired_out[a] = d;
        group_out[a] = (int)base + ldv(s.label + a);
    }
    __syncthreads();
    find_valid_update<kDecideThreads>(s, nullptr, n);
    for (int a = tid; a < n; a += T) write_update(g, !fail && ldv(s.keep + a), desired_out[a], waypoint + (int64_t)a * 3, updated_out + a);
    if (tid == 0 && fail) *s.status = 1;
}

// ---- the WIDE form of the decision (lscqp_waypoints_wide_device) ---------------------------------------------------------------------------
// The same decision spread over the device, stage by stage, each stage a launch of its own that hands its results to the next at the kernel
// boundary; no kernel waits for another workgroup and the number of launches depends on the sign of the range alone:
//   gather (above)
//   groups     range > 0 only: a cell list over the positions (zero, histogram, scan, scatter: a counting sort by x-y cell whose side is at
//              least 1.0001 * range, so a pair the test accepts lies in the same or an adjacent cell), a lock-free union-find over the pairs of
//              the 3 x 3 cells that pass the UNCHANGED test -- the root with the larger id is hooked under the smaller, so a component's root
//              is its least id, the label of the one-workgroup kernel -- and a flatten pass, which also counts the members
//   order      segment offsets per group of more than one agent (one scan over the roots); agents alone decide and filter by themselves,
//              the others drop a key (init_d descending, id descending) into their group's segment
//   walk       one workgroup per group of more than one agent: a bitonic sort of the segment by all lanes, then ONE wavefront runs
//              pibt_walk over node tables of the group's own -- an open-addressed table of 4 n_g .. 8 n_g slots (KeyedTables), in LDS for
//              small groups and in the group's slab of an O(n) buffer otherwise -- with a bound of 4 n_g + 16 passes, then all lanes run
//              the update filter and its fixed point for the members
//   apply      the updates, unless some group reached its bound
// Keys are distinct and every table answers the same whatever slot an entry landed in, so no result depends on the order in which atomics
// arrive.  Every work array is written before it is read within the call: nothing has to be left clean.
constexpr int kWideThreads = 256;
constexpr int kWideLdsKeys = 1024;  // a segment of up to this many agents is sorted in LDS
constexpr int kWideLdsCap = 1024;   // ... and a node table of up to this many slots (n_g <= 256) lives there

struct Cells {  // the cell list's geometry, from the host
    double side;
    int ncx, ncy;
};

struct Wide {  // work arrays of the wide form (lscqp_grid_reserve_wide), every size a function of n alone
    float4* sorted;       // [n]          position and id of the agents, cell by cell
    uint64_t* keys;       // [n]          sort keys, one segment per group
    int32_t *segstart, *fill, *grouplist;  // [n] each: a root's segment start and fill cursor; the roots of the groups to walk
    int32_t *cell_count, *cell_fill, *cell_start;  // [2 n + 17] each
    int32_t* table;       // [24 n]       a group's slab starts at 24 * segstart: key, now, next of up to 8 n_g slots
    int32_t* misc;        // [0] groups to walk, [1] some group reached its bound
};

__device__ __forceinline__ int ald(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int cell_of(const Cells& c, const View& g, float px, float py) {
#pragma clang fp contract(off)
    const double fx = floor(((double)px - g.gmin0) / c.side), fy = floor(((double)py - g.gmin1) / c.side);
    const int cx = (int)fmin(fmax(fx, 0.0), (double)(c.ncx - 1)), cy = (int)fmin(fmax(fy, 0.0), (double)(c.ncy - 1));  // (outside the box, NaN: an edge cell)
    return cy * c.ncx + cx;
}

// exclusive scan of one value per lane over a workgroup of T lanes; *total: the sum
template <int T>
__device__ __forceinline__ int block_scan(int v, int* sh, int* total) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int off = 1; off < T; off <<= 1) {
        const int t = tid >= off ? sh[tid - off] : 0;
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    const int incl = sh[tid];
    *total = sh[T - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(256) void wide_zero_kernel(int count, int32_t* __restrict__ p, int32_t* __restrict__ q) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id < count) p[id] = 0, q[id] = 0;
}

__global__ __launch_bounds__(256) void cell_count_kernel(View g, Cells c, int n, const double* __restrict__ state, Wide w) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= n) return;
    atomicAdd(w.cell_count + cell_of(c, g, (float)state[(int64_t)a * 9], (float)state[(int64_t)a * 9 + 1]), 1);
}

// cell_start[0..ncell]: the exclusive scan of the counts, by one workgroup (ncell <= 2 n + 16)
__global__ __launch_bounds__(1024) void cell_scan_kernel(int ncell, Wide w) {
    __shared__ int sh[1024];
    const int tid = threadIdx.x, per = (ncell + 1023) / 1024, lo = min(tid * per, ncell), hi = min(lo + per, ncell);
    int sum = 0;
    for (int i = lo; i < hi; i++) sum += w.cell_count[i];
    int total;
    int run = block_scan<1024>(sum, sh, &total);
    for (int i = lo; i < hi; i++) {
        w.cell_start[i] = run;
        run += w.cell_count[i];
    }
    if (tid == 0) w.cell_start[ncell] = total;
}

__global__ __launch_bounds__(256) void cell_scatter_kernel(View g, Cells c, int n, const double* __restrict__ state, Wide w) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= n) return;
    const float px = (float)state[(int64_t)a * 9], py = (float)state[(int64_t)a * 9 + 1], pz = (float)state[(int64_t)a * 9 + 2];
    const int cell = cell_of(c, g, px, py);
    const int slot = w.cell_start[cell] + atomicAdd(w.cell_fill + cell, 1);
    if (slot >= 0 && slot < n) w.sorted[slot] = make_float4(px, py, pz, __int_as_float(a));
}

// union-find over the parent array `par` (the labels): every access is an agent-scope atomic, parents only fall and stay inside the component
__device__ __forceinline__ int uf_find(int32_t* par, int x) {
    for (;;) {
        const int p = ald(par + x);
        if (p == x) return x;
        const int gp = ald(par + p);
        if (gp < p) __hip_atomic_fetch_min(par + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (path halving)
        x = p;
    }
}

__global__ __launch_bounds__(256) void hook_kernel(View g, Cells c, int n, double range, Wide w, int32_t* par) {
#pragma clang fp contract(off)
    const int slot = blockIdx.x * 256 + threadIdx.x;
    if (slot >= n) return;
    const float4 me = w.sorted[slot];
    const int a = __float_as_int(me.w);
    if (a < 0 || a >= n) return;  // (never: the scatter filled every slot)
    const int lo = cell_of(c, g, me.x, me.y);
    const int cy = lo / c.ncx, cx = lo - cy * c.ncx;
    for (int yy = max(cy - 1, 0); yy <= min(cy + 1, c.ncy - 1); yy++)
        for (int xx = max(cx - 1, 0); xx <= min(cx + 1, c.ncx - 1); xx++) {
            const int cell = yy * c.ncx + xx, b = max(w.cell_start[cell], 0), e = min(w.cell_start[cell + 1], n);
            for (int t = b; t < e; t++) {
                const float4 o = w.sorted[t];
                const int j = __float_as_int(o.w);
                if (j >= a || j < 0) continue;  // (every pair once, by its larger id)
                const double d0 = fabs((double)(me.x - o.x)), d1 = fabs((double)(me.y - o.y)), d2 = fabs((double)(me.z - o.z));
                if (!(fmax(d0, fmax(d1, d2)) < range)) continue;
                int ra = uf_find(par, a), rb = uf_find(par, j);
                while (ra != rb) {  // hook the root with the larger id under the smaller
                    const int big = max(ra, rb), small = min(ra, rb);
                    int expect = big;
                    if (__hip_atomic_compare_exchange_strong(par + big, &expect, small, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
                    ra = uf_find(par, big), rb = uf_find(par, small);
                }
            }
        }
}

// every agent's label becomes its root (roots do not move here: whatever a lane reads on the way is an ancestor); the roots count their members
__global__ __launch_bounds__(256) void flatten_kernel(int n, Scratch s) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= n) return;
    int x = a;
    for (int p = ald(s.label + x); p != x; p = ald(s.label + x)) x = p;
    __hip_atomic_store(s.label + a, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    atomicAdd(s.gsize + x, 1);
}

// one workgroup: the groups of more than one agent in the order of their roots -- segstart[root], grouplist[k] = root, misc[0] = their number
__global__ __launch_bounds__(1024) void segments_kernel(int n, Scratch s, Wide w) {
    __shared__ int sh[1024];
    const int tid = threadIdx.x, per = (n + 1023) / 1024, lo = min(tid * per, n), hi = min(lo + per, n);
    int members = 0, groups = 0;
    for (int a = lo; a < hi; a++) {
        const int sz = s.label[a] == a ? s.gsize[a] : 0;
        if (sz > 1) members += sz, groups++;
    }
    int total_members, total_groups;
    int run_m = block_scan<1024>(members, sh, &total_members), run_g = block_scan<1024>(groups, sh, &total_groups);
    for (int a = lo; a < hi; a++) {
        const int sz = s.label[a] == a ? s.gsize[a] : 0;
        w.fill[a] = 0;
        w.segstart[a] = run_m;
        if (sz > 1) {
            w.grouplist[run_g++] = a;
            run_m += sz;
        }
    }
    if (tid == 0) w.misc[0] = total_groups, w.misc[1] = 0;
}

// agents alone in their group decide and filter by themselves (nobody can hold their node: blocker stays -1); the others drop their key --
// ascending keys are init_d descending, then id descending, PIBT's priority at the first timestep -- into their group's segment
__global__ __launch_bounds__(256) void place_kernel(View g, int n, double range, int M, int dim, const double* __restrict__ state,
                                                    const double* __restrict__ plan, const double* __restrict__ cur_goal,
                                                    const int32_t* __restrict__ init_d, const double* waypoint, Scratch s, Wide w,
                                                    int32_t* __restrict__ group_out, int32_t* __restrict__ desired_out) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= n) return;
    const int la = s.label[a];
    if (s.gsize[la] == 1) {
        const int v = choose_alone(s, a), d = v < 0 ? s.cur[a] : v;
        s.vnext[a] = d;
        s.keep[a] = filter_abc(g, range, M, dim, state, plan, cur_goal, waypoint, a, d);
        desired_out[a] = d;
        group_out[a] = la;
        return;
    }
    const int slot = w.segstart[la] + atomicAdd(w.fill + la, 1);
    if (slot >= 0 && slot < n) w.keys[slot] = ((uint64_t)(~((uint32_t)init_d[a] ^ 0x80000000u)) << 32) | (uint32_t)~(uint32_t)a;
}

__device__ __forceinline__ void key_swap(uint64_t* kk, int i, int j) {
    const uint64_t x = kk[i], y = kk[j];
    if (y < x) kk[i] = y, kk[j] = x;
}

// one workgroup per group of more than one agent; agent ids are global throughout
__global__ __launch_bounds__(kWideThreads) void wide_walk_kernel(View g, int n, double range, int M, int dim, const double* __restrict__ state,
                                                                 const double* __restrict__ plan, const double* __restrict__ cur_goal,
                                                                 const double* waypoint, Scratch s, Wide w, int32_t* __restrict__ group_out,
                                                                 int32_t* __restrict__ desired_out) {
    __shared__ uint64_t keys_sh[kWideLdsKeys];
    __shared__ int32_t table_sh[3 * kWideLdsCap];
    __shared__ int fail_sh;
    if ((int)blockIdx.x >= w.misc[0]) return;
    const int tid = threadIdx.x, T = kWideThreads;
    const int root = w.grouplist[blockIdx.x], gs = w.segstart[root], ng = s.gsize[root];
    if (root < 0 || root >= n || ng < 2 || gs < 0 || gs > n - ng) return;  // (never: the segments are the scan of these sizes)
    // -- the order: the segment's keys ascending, by a bitonic network whose comparators all point the same way -- the slots from ng up to the
    // next power of two hold keys larger than any and never move, so a comparator that reaches one is skipped
    uint64_t* kk = w.keys + gs;
    if (ng <= kWideLdsKeys) {
        for (int i = tid; i < ng; i += T) keys_sh[i] = kk[i];
        kk = keys_sh;
    }
    if (tid == 0) fail_sh = 0;
    __syncthreads();
    int p2 = 1;
    while (p2 < ng) p2 <<= 1;
    for (int size = 2; size <= p2; size <<= 1) {
        const int half = size >> 1;
        for (int t = tid; t < (p2 >> 1); t += T) {
            const int blk = t / half, off = t - blk * half, i = blk * size + off, j = blk * size + size - 1 - off;
            if (j < ng) key_swap(kk, i, j);
        }
        __syncthreads();
        for (int stride = half >> 1; stride >= 1; stride >>= 1) {
            for (int t = tid; t < (p2 >> 1); t += T) {
                const int i = 2 * stride * (t / stride) + t % stride, j = i + stride;
                if (j < ng) key_swap(kk, i, j);
            }
            __syncthreads();
        }
    }
    int32_t* order = s.order + gs;
    for (int i = tid; i < ng; i += T) order[i] = (int)~(uint32_t)kk[i];
    // -- the group's node tables: slots for the members' nodes and the nodes they take, at most half full
    int cap = 8;
    while (cap < 4 * ng) cap <<= 1;
    const unsigned mask = (unsigned)cap - 1u;
    int32_t* tkey = cap <= kWideLdsCap ? table_sh : w.table + 24 * (int64_t)gs;
    int32_t *now = tkey + cap, *next = now + cap;
    for (int i = tid; i < cap; i += T) tkey[i] = -1, now[i] = 0, next[i] = 0;
    __syncthreads();
    // -- PIBT::run's planning loop for the first timestep over this group, by ONE wavefront: the walk of decide_kernel, the node tables looked up
    // by key, with a bound of this group's own
    if (tid < 64) {
        const int lane = tid;
        const KeyedTables t{tkey, now, next, mask};
        for (int idx = lane; idx < ng; idx += 64) {  // occupied_now: the last id wins
            const int a = order[idx], node = s.cur[a];
            for (unsigned h = table_hash(node, mask), probes = 0; probes <= mask; h = (h + 1) & mask, probes++) {
                const int was = atomicCAS(tkey + h, -1, node);
                if (was == -1 || was == node) {
                    atomicMax(now + h, a + 1);
                    break;
                }
            }
        }
        __threadfence_block();
        __builtin_amdgcn_wave_barrier();
        int passes = 0;
        const int fail = pibt_walk(s, t, order, ng, s.stack + gs, lane, passes, 4 * ng + 16);
        if (fail && lane == 0) {
            fail_sh = 1;
            __hip_atomic_store(w.misc + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    // -- the update filter for the members: (a)-(c), then "find valid update" -- `blocker` is a member, the fixed point stays in the group
    for (int i = tid; i < ng; i += T) {
        const int a = order[i], vn = ldv(s.vnext + a), d = vn < 0 ? s.cur[a] : vn;
        stv(s.keep + a, filter_abc(g, range, M, dim, state, plan, cur_goal, waypoint, a, d));
        desired_out[a] = d;
        group_out[a] = root;
    }
    __syncthreads();
    find_valid_update<kWideThreads>(s, order, ng);
}

__global__ __launch_bounds__(256) void apply_kernel(View g, int n, Scratch s, Wide w, const int32_t* __restrict__ desired, double* __restrict__ waypoint,
                                                    int32_t* __restrict__ updated_out) {
#pragma clang fp contract(off)
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= n) return;
    const int fail = w.misc[1];
    write_update(g, !fail && s.keep[a], desired[a], waypoint + (int64_t)a * 3, updated_out + a);
    if (a == 0 && fail) *s.status = 1;
}

}  // namespace lscgrid

struct lscqp_grid_s {
    lscgrid::View v;
    double radius = 0, gmin[3] = {0, 0, 0};
    int dims[3] = {0, 0, 0};
    int device = 0;
    lscqp::dev_ptr<uint8_t> d_occ, d_occ_mission;
    int64_t reserved = 0;
    lscqp::dev_ptr<int32_t> d_agent_scratch;  // 11 arrays, the candidate ones five wide
    lscqp::dev_ptr<int32_t> d_tables;         // now, next, status
    lscgrid::Scratch s;
    // a mission partition (lscqp_grid_reserve_missions_): one occupancy copy and one status word per mission, and where the node tables do
    // not fit in LDS one slab of them per mission
    int missions = 0;
    lscqp::dev_ptr<uint8_t> d_occ_k;     // [missions][nodes]
    lscqp::dev_ptr<int32_t> d_status_k;  // [missions]
    lscqp::dev_ptr<int32_t> d_tables_k;  // [missions][2][nodes], all zero between launches
    std::vector<int64_t> fields_off;  // the partition of the last lscqp_grid_fields_missions_device: the one the copies were cleared for
    // a base occupancy per world (lscqp_grid_set_worlds): mission k's copy starts from base k; 0 = the one base d_occ
    int worlds = 0;
    lscqp::dev_ptr<uint8_t> d_occ_w;  // [worlds][nodes]
    // the wide form of the decision (lscqp_grid_reserve_wide)
    int64_t wide_reserved = 0;
    lscqp::dev_ptr<char> d_wide;
    lscgrid::Wide w;
};

namespace {

// a failed call answers with its own text; an allocation (lscqp::dev_alloc) names the hipMalloc it makes in the same way
#define GRID_HIP(call)                                            \
    do {                                                          \
        const hipError_t e_ = (call);                             \
        if (e_ != hipSuccess) return lscqp::hip_fail(e_, #call);  \
    } while (0)

constexpr int64_t kPerAgentInts = 9 + 2 * 5;  // cur, vnext, order, stack, label, blocker, keep, onnode, gsize + cand[5], cost[5]

// what the one-mission entries answer on a grid with a base occupancy per world (lscqp_grid_set_worlds)
const char* const kOneMissionOverWorlds =
    "the grid has a base occupancy per world (lscqp_grid_set_worlds): the one-mission entries have no single base to read -- use the "
    "_missions_ entries with one mission per world, or lscqp_grid_set_worlds(grid, NULL)";

bool tables_fit_lds(const lscqp_grid_s* g) {
    return (size_t)2 * g->dims[0] * g->dims[1] * sizeof(int32_t) <= (size_t)lscgrid::kTableLdsBytes;
}

// the argument checks the three lscqp_waypoints_* entries share.  `entry`: the caller's own name; `buffers`: the device pointers that must
// not be null -- where `need_buffers` says so (the single-swarm entries take null buffers with no agents) -- refused with `null_msg`
int check_waypoint_args(const char* entry, lscqp_grid g, int64_t n, bool need_buffers, std::initializer_list<const void*> buffers, const char* null_msg,
                        double communication_range, int32_t M, int32_t dim, const double* d_plan) {
    if (!g || n < 0) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "bad argument");
    if (need_buffers)
        for (const void* p : buffers)
            if (!p) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, null_msg);
    if (dim != 2) return lscqp_set_error_(LSCQP_ERR_UNSUPPORTED, (std::string(entry) + " is 2-D only").c_str());
    if (d_plan && M < 1) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "M must be positive");
    if (!(communication_range == communication_range)) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "communication_range is NaN");
    return LSCQP_OK;
}

// one workgroup per agent relaxes its field: in LDS where the padded grid fits, in HBM otherwise (d_off: the mission partition, or null)
void launch_fields(const lscqp_grid_s* g, int64_t n, const uint8_t* occ, const double* d_start_points, const double* d_goal_points, int32_t* d_field,
                   int32_t* d_init_d, const int64_t* d_off, int K, hipStream_t st) {
    const int64_t padded = (int64_t)(g->dims[0] + 2) * (g->dims[1] + 2);
    if (padded <= lscgrid::kLdsNodes) {
        const int threads = padded <= 2048 ? 256 : 1024;
        const size_t lds = (size_t)((padded * 2 + 15) / 16 * 16);
        hipLaunchKernelGGL(lscgrid::fields_kernel<true>, dim3((unsigned)n), dim3(threads), lds, st, g->v, occ, d_start_points, d_goal_points, d_field, d_init_d, d_off, K);
    } else {
        hipLaunchKernelGGL(lscgrid::fields_kernel<false>, dim3((unsigned)n), dim3(1024), 0, st, g->v, occ, d_start_points, d_goal_points, d_field, d_init_d, d_off, K);
    }
}

}  // namespace

extern "C" {

int lscqp_grid_shape(const double* world_min, const double* world_max, double resolution, int32_t world_dimension, double z_2d, double* grid_min,
                     int32_t* dims) {
    if (!world_min || !world_max || !grid_min || !dims) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null argument");
    if (!(resolution > 0)) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "grid resolution must be positive");
    if (world_dimension != 2 && world_dimension != 3) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "world_dimension must be 2 or 3");
    double gmax[3];
    for (int i = 0; i < 3; i++) {  // updateGridInfo (src/grid_based_planner.cpp:86-100), SP_EPSILON = 1e-9
        const double lo = floor((-world_min[i] + 1e-9) / resolution), hi = floor((world_max[i] + 1e-9) / resolution);
        grid_min[i] = -lo * resolution;
        gmax[i] = hi * resolution;
    }
    if (world_dimension == 2) grid_min[2] = gmax[2] = z_2d;
    for (int i = 0; i < 3; i++) {
        const double span = (gmax[i] - grid_min[i]) / resolution;
        if (!(span >= 0) || span > 1e6) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "the world box is empty or the grid has more than 1e6 nodes per axis");
        dims[i] = (int32_t)round(span) + 1;
    }
    return LSCQP_OK;
}

int lscqp_grid_create(lscqp_map map, const lscqp_grid_desc* desc, lscqp_grid* out) {
    if (!map || !desc || !out) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null argument");
    if (desc->world_dimension != 2)
        return lscqp_set_error_(LSCQP_ERR_UNSUPPORTED,
                                "lscqp_grid is 2-D only: the reference's MAPF graph is x-y (Grid::Grid) and its 3-D waypoints come out at the floor of the world");
    if (!(desc->resolution > 0) || !(desc->radius >= 0)) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "grid resolution must be positive and radius non-negative");
    double res = 0;
    float wmin[3], wmax[3];
    int key0[3], mdims[3], mdev = 0;
    const int32_t* nearest = nullptr;
    lscqp_map_raw_(map, &res, wmin, wmax, key0, mdims, &nearest, &mdev);
    int cur_dev = 0;
    if (hipGetDevice(&cur_dev) != hipSuccess) return lscqp_set_error_(LSCQP_ERR_NO_DEVICE, "no HIP device: lscqp has no CPU fallback");
    if (mdev != cur_dev) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "the map lives on another device than the current one");
    const double wmin_d[3] = {wmin[0], wmin[1], wmin[2]}, wmax_d[3] = {wmax[0], wmax[1], wmax[2]};  // (mission.world_min / _max are point3d)
    std::unique_ptr<lscqp_grid_s> g(new lscqp_grid_s());
    if (const int rc = lscqp_grid_shape(wmin_d, wmax_d, desc->resolution, 2, desc->z_2d, g->gmin, g->dims)) return rc;
    if ((int64_t)g->dims[0] * g->dims[1] > (int64_t)1 << 26) return lscqp_set_error_(LSCQP_ERR_UNSUPPORTED, "more than 2^26 grid nodes");
    g->device = cur_dev;
    g->radius = desc->radius;
    g->v = lscgrid::View{g->gmin[0], g->gmin[1], desc->resolution, desc->z_2d, g->dims[0], g->dims[1]};
    const lscgrid::MapRaw mraw{res, key0[0], key0[1], key0[2], mdims[0], mdims[1], mdims[2], nearest};  // (read by the occupancy kernel below and not kept: the grid outlives its map)
    const int nodes = g->dims[0] * g->dims[1];
    const char* const what = "lscqp_grid_create";
    if (const int rc = lscqp::dev_alloc(g->d_occ, (size_t)nodes, what)) return rc;
    if (const int rc = lscqp::dev_alloc(g->d_occ_mission, (size_t)nodes, what)) return rc;
    if (const int rc = lscqp::dev_alloc(g->d_tables, (size_t)2 * nodes + 4, what, true)) return rc;
    hipLaunchKernelGGL(lscgrid::occupancy_kernel, dim3((unsigned)((nodes + 255) / 256)), dim3(256), 0, (hipStream_t)0, g->v, mraw, g->radius, g->d_occ.get());
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(g->d_occ_mission.get(), g->d_occ.get(), (size_t)nodes, hipMemcpyDeviceToDevice);
    // (the LDS form of the field kernel may ask for more than the 64 KB a kernel gets by default)
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&lscgrid::fields_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, lscgrid::kLdsNodes * 2);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return lscqp::hip_fail(e, what);
    *out = g.release();
    return LSCQP_OK;
}

void lscqp_grid_destroy(lscqp_grid g) {
    if (!g) return;
    lscqp::OnDevice on(g->device);
    (void)hipDeviceSynchronize();
    delete g;
}

int lscqp_grid_info(lscqp_grid g, double* grid_min, int32_t* dims) {
    if (!g || !grid_min || !dims) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null argument");
    for (int k = 0; k < 3; k++) grid_min[k] = g->gmin[k], dims[k] = g->dims[k];
    return LSCQP_OK;
}

int lscqp_grid_download(lscqp_grid g, uint8_t* occ) {
    if (!g || !occ) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null argument");
    GRID_HIP(hipMemcpy(occ, g->d_occ.get(), (size_t)g->dims[0] * g->dims[1], hipMemcpyDeviceToHost));
    return LSCQP_OK;
}

int lscqp_grid_download_mission(lscqp_grid g, uint8_t* occ) {
    if (!g || !occ) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null argument");
    GRID_HIP(hipMemcpy(occ, g->d_occ_mission.get(), (size_t)g->dims[0] * g->dims[1], hipMemcpyDeviceToHost));
    return LSCQP_OK;
}

int lscqp_grid_status(lscqp_grid g, int32_t* status_out) {
    if (!g || !status_out) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null argument");
    GRID_HIP(hipMemcpy(status_out, g->d_tables.get() + (size_t)2 * g->dims[0] * g->dims[1], sizeof(int32_t), hipMemcpyDeviceToHost));
    return LSCQP_OK;
}

int lscqp_grid_reserve(lscqp_grid g, int64_t n) {
    if (!g || n < 0) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "bad argument");
    if (n > ((int64_t)1 << 24)) return lscqp_set_error_(LSCQP_ERR_UNSUPPORTED, "more than 2^24 agents");
    if (n > g->reserved) {
        GRID_HIP(hipDeviceSynchronize());
        g->reserved = 0;
        if (const int rc = lscqp::dev_alloc(g->d_agent_scratch, (size_t)n * kPerAgentInts, "hipMalloc((void**)&g->d_agent_scratch, (size_t)n * kPerAgentInts * sizeof(int32_t))")) return rc;
        g->reserved = n;
    }
    int32_t* b = g->d_agent_scratch.get();
    const int64_t r = g->reserved;
    lscgrid::Scratch& s = g->s;
    s.cur = b, s.vnext = b + r, s.order = b + 2 * r, s.stack = b + 3 * r, s.label = b + 4 * r, s.blocker = b + 5 * r, s.keep = b + 6 * r;
    s.onnode = b + 7 * r, s.gsize = b + 8 * r, s.cand = b + 9 * r, s.cost = b + 14 * r;
    const int64_t nodes = (int64_t)g->dims[0] * g->dims[1];
    s.now = g->d_tables.get(), s.next = s.now + nodes, s.status = s.now + 2 * nodes;
    return LSCQP_OK;
}

int lscqp_grid_fields_device(lscqp_grid g, int64_t n, const double* d_start_points, const double* d_goal_points, int32_t* d_field, int32_t* d_init_d,
                             void* stream) {
    if (!g || n < 0 || (n > 0 && (!d_start_points || !d_goal_points || !d_field || !d_init_d)))
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "bad argument");
    if (g->worlds) return lscqp_set_error_(LSCQP_ERR_UNSUPPORTED, kOneMissionOverWorlds);
    if (n == 0) return LSCQP_OK;
    hipStream_t st = (hipStream_t)stream;
    const int nodes = g->dims[0] * g->dims[1];
    GRID_HIP(hipMemcpyAsync(g->d_occ_mission.get(), g->d_occ.get(), (size_t)nodes, hipMemcpyDeviceToDevice, st));
    GRID_HIP(hipMemsetAsync(g->d_tables.get() + (size_t)2 * nodes, 0, 4 * sizeof(int32_t), st));  // a new mission: the status word starts at 0
    hipLaunchKernelGGL(lscgrid::clear_nodes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g->v, n, d_start_points, d_goal_points, g->d_occ_mission.get(),
                       (const int64_t*)nullptr, 0);
    launch_fields(g, n, g->d_occ_mission.get(), d_start_points, d_goal_points, d_field, d_init_d, nullptr, 0, st);
    GRID_HIP(hipGetLastError());
    return LSCQP_OK;
}

int lscqp_waypoints_device(lscqp_grid g, double communication_range, int32_t M, int32_t dim, int64_t n, const double* d_state, const double* d_plan,
                           const double* d_current_goal, const int32_t* d_field, const int32_t* d_init_d, double* d_waypoint, int32_t* d_group_out,
                           int32_t* d_desired_out, int32_t* d_updated_out, void* stream) {
    {
        const int rc = check_waypoint_args("lscqp_waypoints_device", g, n, n > 0, {d_state, d_current_goal, d_field, d_init_d, d_waypoint, d_group_out, d_desired_out, d_updated_out},
                                           "bad argument", communication_range, M, dim, d_plan);
        if (rc != LSCQP_OK) return rc;
    }
    if (g->worlds) return lscqp_set_error_(LSCQP_ERR_UNSUPPORTED, kOneMissionOverWorlds);
    if (n == 0) return LSCQP_OK;
    if (n > g->reserved) {  // (synchronises and allocates: a caller that captures the launch reserves beforehand)
        const int rc = lscqp_grid_reserve(g, n);
        if (rc != LSCQP_OK) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    const int nodes = g->dims[0] * g->dims[1];
    hipLaunchKernelGGL(lscgrid::gather_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g->v, n, communication_range, g->d_occ_mission.get(), d_waypoint, d_field, g->s,
                       (const int64_t*)nullptr, 0);
    const size_t table_bytes = (size_t)2 * nodes * sizeof(int32_t);
    const int in_lds = table_bytes <= (size_t)lscgrid::kTableLdsBytes;
    hipLaunchKernelGGL(lscgrid::decide_kernel<false>, dim3(1), dim3(lscgrid::kDecideThreads), in_lds ? (table_bytes + 15) / 16 * 16 : 0, st, g->v, n, communication_range,
                       (int)M, (int)dim, in_lds, d_state, d_plan, d_current_goal, d_init_d, d_waypoint, g->s, d_group_out, d_desired_out, d_updated_out,
                       (const int64_t*)nullptr);
    GRID_HIP(hipGetLastError());
    return LSCQP_OK;
}

int lscqp_grid_reserve_wide(lscqp_grid g, int64_t n) {
    if (!g || n < 0) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "bad argument");
    {
        const int rc = lscqp_grid_reserve(g, n);
        if (rc != LSCQP_OK) return rc;
    }
    if (n <= g->wide_reserved) return LSCQP_OK;
    GRID_HIP(hipDeviceSynchronize());
    g->wide_reserved = 0;
    const size_t r = (size_t)n, cells = 2 * r + 17;
    const size_t ints = 3 * r + 3 * cells + 24 * r + 4;
    if (const int rc = lscqp::dev_alloc(g->d_wide, r * sizeof(float4) + r * sizeof(uint64_t) + ints * sizeof(int32_t),
                              "hipMalloc(&g->d_wide, r * sizeof(float4) + r * sizeof(uint64_t) + ints * sizeof(int32_t))")) return rc;
    lscgrid::Wide& w = g->w;
    w.sorted = (float4*)g->d_wide.get();
    w.keys = (uint64_t*)(w.sorted + r);
    int32_t* b = (int32_t*)(w.keys + r);
    w.segstart = b, w.fill = b + r, w.grouplist = b + 2 * r;
    w.cell_count = b + 3 * r, w.cell_fill = w.cell_count + cells, w.cell_start = w.cell_fill + cells;
    w.table = w.cell_start + cells;
    w.misc = w.table + 24 * r;
    g->wide_reserved = n;
    return LSCQP_OK;
}

int lscqp_waypoints_wide_device(lscqp_grid g, double communication_range, int32_t M, int32_t dim, int64_t n, const double* d_state, const double* d_plan,
                                const double* d_current_goal, const int32_t* d_field, const int32_t* d_init_d, double* d_waypoint, int32_t* d_group_out,
                                int32_t* d_desired_out, int32_t* d_updated_out, void* stream) {
    {
        const int rc = check_waypoint_args("lscqp_waypoints_wide_device", g, n, n > 0, {d_state, d_current_goal, d_field, d_init_d, d_waypoint, d_group_out, d_desired_out, d_updated_out},
                                           "bad argument", communication_range, M, dim, d_plan);
        if (rc != LSCQP_OK) return rc;
    }
    if (g->worlds) return lscqp_set_error_(LSCQP_ERR_UNSUPPORTED, kOneMissionOverWorlds);
    if (n == 0) return LSCQP_OK;
    if (n > g->wide_reserved || n > g->reserved) {  // (synchronises and allocates: a caller that captures the launch reserves beforehand)
        const int rc = lscqp_grid_reserve_wide(g, n);
        if (rc != LSCQP_OK) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    const double range = communication_range;
    const int ni = (int)n;
    const dim3 per_agent((unsigned)((n + 255) / 256)), b256(256);
    const lscgrid::Scratch& s = g->s;
    const lscgrid::Wide& w = g->w;
    hipLaunchKernelGGL(lscgrid::gather_kernel<false>, per_agent, b256, 0, st, g->v, n, range, g->d_occ_mission.get(), d_waypoint, d_field, s, (const int64_t*)nullptr, 0);
    if (range > 0) {
        // the cell side: the range and a margin for the rounding of the float32 subtraction in the test, enlarged until 2 n + 16 cells cover the
        // grid's box (positions outside fall into the edge cells)
        const double lx = (g->dims[0] - 1) * g->v.res, ly = (g->dims[1] - 1) * g->v.res, limit = 2.0 * (double)n + 16.0;
        lscgrid::Cells c;
        c.side = 1.0001 * range;
        while ((floor(lx / c.side) + 1.0) * (floor(ly / c.side) + 1.0) > limit) c.side *= 1.25;
        c.ncx = (int)floor(lx / c.side) + 1, c.ncy = (int)floor(ly / c.side) + 1;
        const int ncell = c.ncx * c.ncy;
        hipLaunchKernelGGL(lscgrid::wide_zero_kernel, dim3((unsigned)((ncell + 1 + 255) / 256)), b256, 0, st, ncell + 1, w.cell_count, w.cell_fill);
        hipLaunchKernelGGL(lscgrid::cell_count_kernel, per_agent, b256, 0, st, g->v, c, ni, d_state, w);
        hipLaunchKernelGGL(lscgrid::cell_scan_kernel, dim3(1), dim3(1024), 0, st, ncell, w);
        hipLaunchKernelGGL(lscgrid::cell_scatter_kernel, per_agent, b256, 0, st, g->v, c, ni, d_state, w);
        hipLaunchKernelGGL(lscgrid::hook_kernel, per_agent, b256, 0, st, g->v, c, ni, range, w, s.label);
    }
    hipLaunchKernelGGL(lscgrid::flatten_kernel, per_agent, b256, 0, st, ni, s);
    hipLaunchKernelGGL(lscgrid::segments_kernel, dim3(1), dim3(1024), 0, st, ni, s, w);
    hipLaunchKernelGGL(lscgrid::place_kernel, per_agent, b256, 0, st, g->v, ni, range, (int)M, (int)dim, d_state, d_plan, d_current_goal, d_init_d,
                       (const double*)d_waypoint, s, w, d_group_out, d_desired_out);
    // (a group to walk has two members or more: n / 2 workgroups at the most, the ones beyond the number of groups return at once)
    hipLaunchKernelGGL(lscgrid::wide_walk_kernel, dim3((unsigned)((n + 1) / 2)), dim3(lscgrid::kWideThreads), 0, st, g->v, ni, range, (int)M, (int)dim, d_state, d_plan,
                       d_current_goal, (const double*)d_waypoint, s, w, d_group_out, d_desired_out);
    hipLaunchKernelGGL(lscgrid::apply_kernel, per_agent, b256, 0, st, g->v, ni, s, w, (const int32_t*)d_desired_out, d_waypoint, d_updated_out);
    GRID_HIP(hipGetLastError());
    return LSCQP_OK;
}

int lscqp_grid_reserve_missions_(lscqp_grid g, int64_t n, int32_t n_missions) {
    if (!g || n < 0 || n_missions < 1) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "bad argument");
    const int rc = lscqp_grid_reserve(g, n);
    if (rc != LSCQP_OK) return rc;
    if (n_missions <= g->missions) return LSCQP_OK;
    const size_t nodes = (size_t)g->dims[0] * g->dims[1], K = (size_t)n_missions;
    GRID_HIP(hipDeviceSynchronize());
    g->d_occ_k.reset(), g->d_status_k.reset(), g->d_tables_k.reset();
    g->missions = 0;
    g->fields_off.clear();  // (the copies are gone)
    if (const int rc = lscqp::dev_alloc(g->d_occ_k, K * nodes, "hipMalloc((void**)&g->d_occ_k, K * nodes)")) return rc;
    if (const int rc = lscqp::dev_alloc(g->d_status_k, K, "hipMalloc((void**)&g->d_status_k, K * sizeof(int32_t))")) return rc;
    GRID_HIP(hipMemset(g->d_status_k.get(), 0, K * sizeof(int32_t)));
    if (!tables_fit_lds(g)) {
        if (const int rc = lscqp::dev_alloc(g->d_tables_k, K * 2 * nodes, "hipMalloc((void**)&g->d_tables_k, K * 2 * nodes * sizeof(int32_t))")) return rc;
        GRID_HIP(hipMemset(g->d_tables_k.get(), 0, K * 2 * nodes * sizeof(int32_t)));
    }
    g->missions = n_missions;
    return LSCQP_OK;
}

// updateGridMap once per world: [n_worlds][nodes] base occupancies by the kernel and the arithmetic of lscqp_grid_create.  Synchronous; the grid
// keeps nothing of the maps.  NULL: back to the one base
int lscqp_grid_set_worlds(lscqp_grid g, lscqp_worlds worlds) {
    if (!g) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null grid");
    if (const int rc = lscqp_need_device_()) return rc;
    lscqp::OnDevice on(g->device);  // (current while the bases are allocated, written and waited for)
    lscqp::dev_ptr<uint8_t> fresh;
    int K = 0;
    if (worlds) {
        K = lscqp_worlds_count_(worlds);
        const int nodes = g->dims[0] * g->dims[1];
        for (int k = 0; k < K; k++) {
            double res = 0;
            float wmin[3], wmax[3];
            int key0[3], mdims[3], mdev = 0;
            const int32_t* nearest = nullptr;
            lscqp_map_raw_(lscqp_worlds_map_(worlds, k), &res, wmin, wmax, key0, mdims, &nearest, &mdev);
            if (k == 0) {  // (the members agree in shape: the first speaks for all)
                if (mdev != g->device) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_grid_set_worlds: the worlds live on another device than the grid");
                const double wmin_d[3] = {wmin[0], wmin[1], wmin[2]}, wmax_d[3] = {wmax[0], wmax[1], wmax[2]};
                double gmin[3];
                int32_t dims[3];
                const int rc = lscqp_grid_shape(wmin_d, wmax_d, g->v.res, 2, g->v.z_2d, gmin, dims);
                if (rc != LSCQP_OK) return rc;
                if (gmin[0] != g->gmin[0] || gmin[1] != g->gmin[1] || dims[0] != g->dims[0] || dims[1] != g->dims[1])
                    return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_grid_set_worlds: the worlds' box gives another grid than this one (world box differs from the grid's map)");
                if (const int rc = lscqp::dev_alloc(fresh, (size_t)K * nodes, "hipMalloc((void**)&fresh, (size_t)K * nodes)")) return rc;
            }
            const lscgrid::MapRaw mraw{res, key0[0], key0[1], key0[2], mdims[0], mdims[1], mdims[2], nearest};
            hipLaunchKernelGGL(lscgrid::occupancy_kernel, dim3((unsigned)((nodes + 255) / 256)), dim3(256), 0, (hipStream_t)0, g->v, mraw, g->radius, fresh.get() + (size_t)k * nodes);
        }
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) return lscqp::hip_fail(e, "lscqp_grid_set_worlds");
    } else {
        GRID_HIP(hipDeviceSynchronize());  // (a launch may still be reading the bases)
    }
    g->d_occ_w = std::move(fresh);
    g->worlds = K;
    g->fields_off.clear();  // (the mission copies were made from other bases: lscqp_grid_fields_missions_device must come again)
    return LSCQP_OK;
}

int lscqp_grid_download_world(lscqp_grid g, int32_t k, uint8_t* occ) {
    if (!g || !occ) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null argument");
    if (k < 0 || k >= g->worlds) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_grid_download_world: the grid has no such world (lscqp_grid_set_worlds)");
    const size_t nodes = (size_t)g->dims[0] * g->dims[1];
    GRID_HIP(hipMemcpy(occ, g->d_occ_w.get() + (size_t)k * nodes, nodes, hipMemcpyDeviceToHost));
    return LSCQP_OK;
}

int lscqp_grid_mission_status(lscqp_grid g, int32_t n_missions, int32_t* status_out) {
    if (!g || !status_out || n_missions < 1) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "bad argument");
    if (n_missions > g->missions) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "the grid has seen no partition of that many missions");
    GRID_HIP(hipMemcpy(status_out, g->d_status_k.get(), (size_t)n_missions * sizeof(int32_t), hipMemcpyDeviceToHost));
    return LSCQP_OK;
}

int lscqp_grid_fields_missions_device(lscqp_grid g, int64_t n, int32_t n_missions, const int64_t* mission_offsets, const int64_t* d_mission_offsets,
                                      const double* d_start_points, const double* d_goal_points, int32_t* d_field, int32_t* d_init_d, void* stream) {
    if (!g || n < 0) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "bad argument");
    {
        const int rc = lscqp_check_missions_(n, n_missions, mission_offsets);
        if (rc != LSCQP_OK) return rc;
    }
    if (!d_mission_offsets || !d_start_points || !d_goal_points || !d_field || !d_init_d) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "null buffer");
    if (g->worlds && n_missions != g->worlds)
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, ("lscqp_grid_fields_missions_device: the grid has " + std::to_string(g->worlds) + " worlds, the partition " +
                                                             std::to_string(n_missions) + " missions: mission k flies over world k").c_str());
    if (n_missions > g->missions || n > g->reserved) {  // (synchronises and allocates)
        const int rc = lscqp_grid_reserve_missions_(g, n, n_missions);
        if (rc != LSCQP_OK) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    const int nodes = g->dims[0] * g->dims[1], K = n_missions;
    g->fields_off.assign(mission_offsets, mission_offsets + K + 1);
    if (g->worlds)  // mission k's copy starts from world k's base
        GRID_HIP(hipMemcpyAsync(g->d_occ_k.get(), g->d_occ_w.get(), (size_t)nodes * K, hipMemcpyDeviceToDevice, st));
    else
        hipLaunchKernelGGL(lscgrid::spread_occupancy_kernel, dim3((unsigned)(((int64_t)nodes * K + 255) / 256)), dim3(256), 0, st, nodes, K, g->d_occ.get(), g->d_occ_k.get());
    GRID_HIP(hipMemsetAsync(g->d_status_k.get(), 0, (size_t)K * sizeof(int32_t), st));  // new missions: their status words start at 0
    hipLaunchKernelGGL(lscgrid::clear_nodes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g->v, n, d_start_points, d_goal_points, g->d_occ_k.get(),
                       d_mission_offsets, K);
    launch_fields(g, n, g->d_occ_k.get(), d_start_points, d_goal_points, d_field, d_init_d, d_mission_offsets, K, st);
    GRID_HIP(hipGetLastError());
    return LSCQP_OK;
}

int lscqp_waypoints_missions_device(lscqp_grid g, double communication_range, int32_t M, int32_t dim, int64_t n, int32_t n_missions,
                                    const int64_t* mission_offsets, const int64_t* d_mission_offsets, const double* d_state, const double* d_plan,
                                    const double* d_current_goal, const int32_t* d_field, const int32_t* d_init_d, double* d_waypoint,
                                    int32_t* d_group_out, int32_t* d_desired_out, int32_t* d_updated_out, void* stream) {
    if (!g || n < 0) return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "bad argument");
    {
        const int rc = lscqp_check_missions_(n, n_missions, mission_offsets);
        if (rc != LSCQP_OK) return rc;
    }
    {
        const int rc = check_waypoint_args("lscqp_waypoints_missions_device", g, n, true,
                                           {d_mission_offsets, d_state, d_current_goal, d_field, d_init_d, d_waypoint, d_group_out, d_desired_out, d_updated_out}, "null buffer",
                                           communication_range, M, dim, d_plan);
        if (rc != LSCQP_OK) return rc;
    }
    // (the occupancy copies are lscqp_grid_fields_missions_device's, cleared for the agents of ITS partition)
    if (g->fields_off.size() != (size_t)n_missions + 1 || !std::equal(g->fields_off.begin(), g->fields_off.end(), mission_offsets))
        return lscqp_set_error_(LSCQP_ERR_INVALID_ARGUMENT, "lscqp_grid_fields_missions_device over this same partition must come first");
    if (n > g->reserved) {  // (synchronises and allocates)
        const int rc = lscqp_grid_reserve(g, n);
        if (rc != LSCQP_OK) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    const int nodes = g->dims[0] * g->dims[1], K = n_missions;
    hipLaunchKernelGGL(lscgrid::gather_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g->v, n, communication_range, g->d_occ_k.get(), d_waypoint, d_field, g->s,
                       d_mission_offsets, K);
    const size_t table_bytes = (size_t)2 * nodes * sizeof(int32_t);
    const int in_lds = tables_fit_lds(g);
    lscgrid::Scratch s = g->s;
    if (!in_lds) s.now = g->d_tables_k.get(), s.next = g->d_tables_k.get() + nodes;
    s.status = g->d_status_k.get();
    hipLaunchKernelGGL(lscgrid::decide_kernel<true>, dim3((unsigned)K), dim3(lscgrid::kDecideThreads), in_lds ? (table_bytes + 15) / 16 * 16 : 0, st, g->v, n,
                       communication_range, (int)M, (int)dim, in_lds, d_state, d_plan, d_current_goal, d_init_d, d_waypoint, s, d_group_out, d_desired_out,
                       d_updated_out, d_mission_offsets);
    GRID_HIP(hipGetLastError());
    return LSCQP_OK;
}

}  // extern "C"
