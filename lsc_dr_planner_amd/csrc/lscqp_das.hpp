// lscqp_das.hpp — the DUAL ACTIVE SET phase of the batched trajectory-QP solver (round 5), gfx950 only.
//
// Why it exists.  The QP of TrajOptimizer::populatebyrow (reference src/traj_optimizer.cpp:216-514) has a CONSTANT Hessian: the jerk
// cost and the terminal pull depend on the class (dt, weights) and on the number of terminal segments only -- never on the agent's
// neighbours.  And a plan's optimum holds very few of its ~1000 rows: on the bench's own batches 61 of the 64 headline QPs
// (BASELINE configs[1]) have NO active row at all -- the optimum is the unconstrained minimiser -- and the other three hold one; the
// dense-maze class (configs[2]) holds <= 4, the 1024 x M10 x 40 class (configs[3]) <= 5 (tools/proto_gi.py, tools/proto_das.py,
// profiles/r05_proto_active_set.txt).  An interior-point method pays 3-13 full iterations (row passes over every row, assembly and
// LDL^T of the reduced system, two substitutions) to find that out.  The dual active-set method of Goldfarb and Idnani starts AT the
// unconstrained minimiser and adds violated rows one at a time:
//
//     min 1/2 c'Hx c + fx'c   over control points  c = cfix + T z  (the equality rows, eliminated as in lscqp_kernel.hpp),   a_i'c >= h_i
//     C = T (T'Hx T)^-1 T'    the COMPLIANCE of the plan: the displacement of every control point per unit multiplier on one of them.
//                             One symmetric P x P table per number of terminal segments, the same for every axis, built on the host
//                             in extended precision when the class is created (lscqp_das_build_tables) -- 7 KB at M = 5.
//     unconstrained optimum   c_u[k] = cfix[k] - c1_k U1 - c2_k U2 + 2 w_t goal_k G1      (three table vectors: no factorisation)
//     one step for row p      w_p = C a_p;   r = S^-1 A'w_p  (S = A'W over the active rows, carried as J = L^-1 of its Cholesky factor:
//                             S^-1 = J'J, two products per step, a row appended when one joins, rotations when one leaves);
//                             dc = w_p - W r;   t = min( min_{r_j > 0} u_j / r_j ,  -slack_p / a_p'dc );   c += t dc,  u -= t r,  u_p += t
//                             t = the second: p joins the active set;  t = the first: row j leaves it and the step is repeated.
//
// The work per QP is one pass over the rows per step (read from HBM the first time; afterwards from LDS in the small-batch form, from
// L2 otherwise) plus a handful of short vector operations: small batches are bound by the chain of memory round trips of their slowest
// instance, large ones by instruction issue at 0.27 of the HBM roof (NOTES.md sections 12-13).  What it returns is a KKT point of the reference's model: primal violation <= 1e-9 m on EVERY row
// (the last pass), multipliers >= 0, exact complementarity, and the reduced stationarity residual verified against the same scale the
// interior-point kernel uses (<= 1e-9) -- after a final "polish" that rebuilds the point from its multipliers and refines them once.
// An instance the phase does not finish (more active rows than its budget, more steps than its budget, a dependent active set, an
// infeasible row system, a failed verification) is LEFT to the interior-point kernel, which runs behind it over the same batch in
// "first pass after the active-set phase" mode (cls.repair == 3) and skips what is already OPTIMAL.  Nothing here is a CPU fallback and
// nothing is approximate: both methods return the optimum of the same strictly convex QP.
//
// Organisation: one workgroup (64 .. 256 threads) per QP, M / dim / end stop / n_obs are run-time values (one kernel for every class);
// row ids:  [LSC rows o*P + cp | interval lo/hi per (axis, cp) | velocity lo/hi | acceleration lo/hi | communication pairs lo/hi],
// selection = the most violated row (raw slack), lowest id on ties: results are reproducible bit for bit from run to run and across
// the kernel's forms (wavefronts per QP, row format, first look peeled or not; built with -ffp-contract=on for that).
//
// This header holds the device side: helpers and the kernel over a batch (das_kernel); the phase on one instance is the text of
// lscqp_das_body.inc, which das_kernel and lscqp_fused.hip's das_pdip_kernel (the phase and the interior-point instance in one launch) include.
// Its code is compiled with fp contraction "on" (a multiply-add fused where the source writes a * b + c in one expression and nowhere
// else) whatever the including translation unit is built with: the phase's results must be the same bits in every launch form.  (A
// scoped push / pop of the setting, #pragma float_control, is ignored by the gfx950 target.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lscqp_kernel.hpp"  // DevClass, KQ
#include "lscqp_launch.hpp"

// (the pragma holds from here to the end of the including translation unit: include this header after everything else)
#pragma clang fp contract(on)

namespace lscqp_das {

using lscqp::DevClass;
using lscqp::KQ;

constexpr double kTolP = 1e-9;      // a row is violated below -1e-9 m of RAW slack (not divided by the row's norm): the interior-point kernel's primal bar
constexpr double kTolD = 1e-9;      // accepted stationarity (scaled like lscqp_info.res_dual)
constexpr int kMaxK = 32;           // active rows the phase can hold (lanes of one wavefront own the rows of the small factor)

// ---- tables, per number of terminal segments ts = 1 .. M:  [U1 (P) | U2 (P) | G1 (P) | C (P x P, symmetric)] --------------------------
__host__ __device__ constexpr size_t table_stride(int M) { return (size_t)(3 + 6 * M) * (size_t)(6 * M); }
__host__ __device__ constexpr int num_pairs(int M, int dim) { return dim * (6 * M + 5 * M + 4 * M + M * (M - 1) / 2); }

// LDS carve of one QP, in doubles.  kmax and n_stage are the CAPACITIES the carve holds (active rows; LSC rows staged per instance); the
// budgets a launch runs with may be smaller.  das_kernel carves at run time from its arguments; the fused kernel (lscqp_fused.hip) carves
// at compile time from its instance's maxima, so that every offset is an immediate and no scalar register holds one.
struct Layout {
    int P, NX, kmax, NPAIR;
    int o_hdr, o_sfc, o_c, o_cu, o_lam, o_plo, o_phi, o_pix, o_W, o_L, o_u, o_r, o_arhs, o_acoef, o_aint, o_red, o_ctl, o_wb, o_dq, o_C, o_rows, o_tl, n_stage, total;
    __host__ __device__ static constexpr Layout make(int M, int dim, int kmax, int cacheC, int stage_rows = 0) {
        Layout s{};
        s.P = 6 * M, s.NX = dim * s.P, s.kmax = kmax, s.NPAIR = num_pairs(M, dim);
        int o = 0;
        auto take = [&](int n) { const int at = o; o += (n + 1) & ~1; return at; };
        s.o_hdr = take(32);
        s.o_sfc = take(6 * M);
        s.o_c = take(3 * s.P), s.o_cu = take(s.NX), s.o_lam = take(s.NX);  // (c_: a third, zero axis in 2-D: row evaluation without a branch on dim)
        s.o_plo = take(s.NPAIR), s.o_phi = take(s.NPAIR), s.o_pix = take((s.NPAIR + 1) / 2);  // two-sided rows: bounds, packed stencil
        s.o_W = take((kmax + 1) * s.NX);      // w_j = C a_j of the active rows; slot k (the next free one) holds the candidate's
        s.o_L = take(kmax * (kmax + 1));
        s.o_u = take(kmax + 1), s.o_r = take(kmax + 4), s.o_arhs = take(kmax + 1);
        s.o_acoef = take(3 * (kmax + 1));
        s.o_aint = take(2 * (kmax + 1) + 2);  // ints: per active row {id, entry0, entry1, entry2} (+ the candidate); entry = axis << 16 | control point
        s.o_red = take(2 * 24);               // cross-wavefront reductions, double buffered; [20, 24): the wavefronts' empty-interval ballots, [44]: w_c
        s.o_ctl = take(8);                    // the step's decision; [4]: w_t
        s.o_wb = take(8);  // world box of the class, then dt and q2s (a kernel argument indexed with a run-time axis would be fetched through vector memory)
        s.o_dq = take(36);  // the objective's coefficient-rounding term (36 doubles as a kernel argument live in 72 scalar registers the kernel does not have)
        s.o_C = take(cacheC ? s.P * s.P : 0);
        s.n_stage = stage_rows;  // LSC rows of the instance kept in LDS after the first pass (SoA nx | ny | nz | b), 0: re-read from L2
        s.o_rows = take(4 * stage_rows);
#ifdef LSCQP_DAS_TIMING
        s.o_tl = take(16);
#endif
        s.total = o;
        return s;
    }
};

// Wave reductions on the DPP network (lscqp_kernel.hpp: ~150 cycles per fp64 value against ~600 for a ds_bpermute butterfly).
__device__ __forceinline__ double wave_max(double v) { return lscqp::wave_max(v); }
__device__ __forceinline__ double wave_min(double v) { return -lscqp::wave_max(-v); }
__device__ __forceinline__ double wave_sum(double v) { return lscqp::wave_sum(v); }
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_min_i32(int v) {
    return min(v, __builtin_amdgcn_update_dpp(2147483647, v, CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ int wave_min_i32(int v) {  // (the scan of lscqp::wave_reduce1 on one register per value instead of two)
    v = dpp_min_i32<0x111, 0xf>(v);
    v = dpp_min_i32<0x112, 0xf>(v);
    v = dpp_min_i32<0x114, 0xf>(v);
    v = dpp_min_i32<0x118, 0xf>(v);
    v = dpp_min_i32<0x142, 0xa>(v);
    v = dpp_min_i32<0x143, 0xc>(v);
    return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ void wave_argmin(double& v, int& id) {  // lexicographic (value, id), ids >= 0: every lane ends with the result
    const double vm = wave_min(v);
    id = wave_min_i32((v == vm) ? id : 2147483647);
    v = vm;
}
// The latency text's reductions: the same trees on DPP steps that need no identity in the destination.  A step of lscqp::dpp_step is five
// instructions -- two moves that put the identity into the destination for the lanes without a source, two DPP moves, the operation --
// and on a path bound by instruction issue the two moves are time (NOTES section 45).
//   row_shr steps of a sum or of a maximum over values >= 0: `bound_ctrl` gives a lane without a source +0.0 and the destination needs no
//   old value.  +0.0 IS the sum's identity in dpp_step, so the sum adds what it added; fmax(v, +0.0) == v == fmax(v, -1e300) for v >= +0.0.
//   The two row_bcast steps write some rows only: the others keep `old`, the identity, as before.
template <class Op, int CTRL>
__device__ __forceinline__ double dpp_step_zero(double v) {  // (a row_shr step; Op's values are >= +0.0, or Op is the sum)
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
    return Op::ap(v, __hiloint2double(hi, lo));
}
struct OpMax0 {  // a maximum over values >= +0.0: the rows a row_bcast step does not write see +0.0
    static __device__ __forceinline__ double id() { return 0.0; }
    static __device__ __forceinline__ double ap(double a, double b) { return fmax(a, b); }
};
template <class OpA, class OpB, class OpC>
__device__ __forceinline__ void wave_reduce3_zero(double& a, double& b, double& c) {  // lscqp::wave_reduce3's tree and operand order
    a = dpp_step_zero<OpA, 0x111>(a), b = dpp_step_zero<OpB, 0x111>(b), c = dpp_step_zero<OpC, 0x111>(c);
    a = dpp_step_zero<OpA, 0x112>(a), b = dpp_step_zero<OpB, 0x112>(b), c = dpp_step_zero<OpC, 0x112>(c);
    a = dpp_step_zero<OpA, 0x114>(a), b = dpp_step_zero<OpB, 0x114>(b), c = dpp_step_zero<OpC, 0x114>(c);
    a = dpp_step_zero<OpA, 0x118>(a), b = dpp_step_zero<OpB, 0x118>(b), c = dpp_step_zero<OpC, 0x118>(c);
    a = lscqp::dpp_step<OpA, 0x142, 0xa>(a), b = lscqp::dpp_step<OpB, 0x142, 0xa>(b), c = lscqp::dpp_step<OpC, 0x142, 0xa>(c);
    a = lscqp::dpp_step<OpA, 0x143, 0xc>(a), b = lscqp::dpp_step<OpB, 0x143, 0xc>(b), c = lscqp::dpp_step<OpC, 0x143, 0xc>(c);
    a = lscqp::bcast63(a), b = lscqp::bcast63(b), c = lscqp::bcast63(c);
}
template <class Op>
__device__ __forceinline__ double wave_reduce1_zero(double v) {
    v = dpp_step_zero<Op, 0x111>(v);
    v = dpp_step_zero<Op, 0x112>(v);
    v = dpp_step_zero<Op, 0x114>(v);
    v = dpp_step_zero<Op, 0x118>(v);
    v = lscqp::dpp_step<Op, 0x142, 0xa>(v);
    v = lscqp::dpp_step<Op, 0x143, 0xc>(v);
    return lscqp::bcast63(v);
}
//   wave_argmin's minimum: zero is not neutral, so the four steps inside a row are rotations (row_ror), in which every lane has a source:
//   every lane of a row ends with the row's minimum, lane 63 behind the two row_bcast steps with the wavefront's.  A minimum is exact under
//   any association (the hardware orders -0.0 below +0.0 in every step), so it is wave_min's value, bit for bit; a NaN is dropped by
//   fmin wherever another value stands beside it, as wave_min's fmax drops it.
struct OpMin {
    static __device__ __forceinline__ double id() { return 1e300; }
    static __device__ __forceinline__ double ap(double a, double b) { return fmin(a, b); }
};
template <int CTRL>
__device__ __forceinline__ double dpp_step_ror_min(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
    return fmin(v, __hiloint2double(hi, lo));
}
__device__ __forceinline__ double wave_min_ror(double v) {
    v = dpp_step_ror_min<0x121>(v);  // row_ror:1
    v = dpp_step_ror_min<0x122>(v);  // row_ror:2
    v = dpp_step_ror_min<0x124>(v);  // row_ror:4
    v = dpp_step_ror_min<0x128>(v);  // row_ror:8
    v = lscqp::dpp_step<OpMin, 0x142, 0xa>(v);
    v = lscqp::dpp_step<OpMin, 0x143, 0xc>(v);
    return lscqp::bcast63(v);
}
__device__ __forceinline__ void wave_argmin_ror(double& v, int& id) {  // wave_argmin with wave_min_ror
    const double vm = wave_min_ror(v);
    id = wave_min_i32((v == vm) ? id : 2147483647);
    v = vm;
}
// a / b for small non-negative integers (a < 2^20, b <= 2^10) through one fp32 multiplication: exact, and a handful of instructions where an
// integer division by a run-time value costs ~40
__device__ __forceinline__ int fdiv(int a, float inv_b) { return (int)(((float)a + 0.5f) * inv_b); }

// LDS hand-overs.  Inside ONE wavefront: its LDS operations execute in order, the fences keep the compiler from moving them.  Across the
// workgroup: s_barrier behind a wait on the LDS counter only -- a __syncthreads() would also wait for every global load in flight, and the
// rows of the first pass are meant to stay in flight across the barriers of the prologue.
#ifndef LSCQP_DAS_FULL_SYNC
#define LSCQP_DAS_WAVE_SYNC()                                   \
    do {                                                        \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  \
        __builtin_amdgcn_wave_barrier();                        \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  \
    } while (0)
#define LSCQP_DAS_BARRIER()                                                           \
    do {                                                                              \
        if constexpr (NW > 1) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); \
        else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                       \
    } while (0)
#else
// The TWIN of the race test (tests/test_race_twin.py; lsc_dr_planner_amd/build.py builds liblscqp_sync.so from this file with
// -DLSCQP_DAS_FULL_SYNC): every hand-over waits for EVERYTHING in flight -- vector memory, LDS, scalar memory -- behind workgroup-scope fences,
// and the workgroup barrier is the compiler's own __syncthreads().  Slower, and by construction free of the one assumption the product's
// hand-overs make (LDS-counter waits only, global loads left in flight); the test demands bit-identical results from both.
#define LSCQP_DAS_WAVE_SYNC()                                           \
    do {                                                                \
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");          \
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");     \
        __builtin_amdgcn_wave_barrier();                                \
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");          \
    } while (0)
#define LSCQP_DAS_BARRIER()                                             \
    do {                                                                \
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");          \
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");     \
        if constexpr (NW > 1) __syncthreads();                          \
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");          \
    } while (0)
#endif

// Development aid: per-phase cycle totals, compiled in only with -DLSCQP_DAS_TIMING (tools/das_timing.py)
#ifdef LSCQP_DAS_TIMING
#ifndef LSCQP_DAS_CYCLES
#define LSCQP_DAS_CYCLES das_cycles  // (the fused translation unit keeps its totals under a name of its own: das_fused_cycles)
#endif
__device__ unsigned long long LSCQP_DAS_CYCLES[16];
// (-DLSCQP_DAS_TIMING_TID=<thread>: the thread of each workgroup that is booked, in the same 16 slots -- 64 books the second wavefront, the
// objective's side of the verification; a probe inside code only wavefront 0 runs then books nothing)
#ifndef LSCQP_DAS_TIMING_TID
#define LSCQP_DAS_TIMING_TID 0
#endif
// (the booked thread -- thread 0 unless LSCQP_DAS_TIMING_TID says otherwise -- accumulates in LDS and adds to the global totals once, at the end: an atomic behind every probe would be waited for by the next
// wait on vector memory -- a round trip of microseconds booked on whatever phase comes next)
#define DAS_T_DECL()                                                                                                                  \
    unsigned long long* const das_tl_ = reinterpret_cast<unsigned long long*>(smem + L.o_tl);                                         \
    if (threadIdx.x == LSCQP_DAS_TIMING_TID)                                                                                          \
        for (int i_ = 0; i_ < 16; i_++) das_tl_[i_] = 0;                                                                              \
    unsigned long long tprev_ = __builtin_readcyclecounter()
#define DAS_T(slot)                                                        \
    do {                                                                   \
        if ((LSCQP_DAS_TIMING >> (slot)) & 1) {                            \
            const unsigned long long now_ = __builtin_readcyclecounter();  \
            if (tid == LSCQP_DAS_TIMING_TID) das_tl_[slot] += now_ - tprev_; \
            tprev_ = now_;                                                 \
        }                                                                  \
    } while (0)
#ifndef LSCQP_DAS_TIMING_MIN_STEPS
#define LSCQP_DAS_TIMING_MIN_STEPS 0  /* only instances with at least that many steps are booked */
#endif
#define DAS_T_FLUSH()                                                                    \
    do {                                                                                 \
        if (tid == LSCQP_DAS_TIMING_TID && steps >= LSCQP_DAS_TIMING_MIN_STEPS)          \
            for (int i_ = 0; i_ < 16; i_++) atomicAdd(&LSCQP_DAS_CYCLES[i_], das_tl_[i_]);   \
    } while (0)
#else
#define DAS_T_DECL() \
    do {             \
    } while (0)
#define DAS_T(slot) \
    do {            \
    } while (0)
#define DAS_T_FLUSH() \
    do {              \
    } while (0)
#endif

// The two texts of the phase (lscqp_das_body.inc, whose header says what the second does differently): the values of LSCQP_DAS_FORM, which
// the including kernel defines.
#define LSCQP_DAS_THROUGHPUT 1  // every value read where it is used, no step setup ahead of the first step: das_kernel, the fused form <10,3,1,10,4>
#define LSCQP_DAS_LATENCY 2     // one instance with steps is the launch's time: the fused forms <5,3,1,5,2> and <10,2,1,5,2>

// The kernel-argument block of a kernel that holds the phase with LSCQP_DAS_FORM LSCQP_DAS_LATENCY: every pointer and class scalar the phase
// reads before its first pass, asked for at kernel entry and waited for ONCE -- in front of the exit test, the order indirection and every branch.  Left where they are used,
// the compiler sinks these reads behind the tests around their uses (a scalar load and a wait of its own per use: seven dependent waits
// up to the first barrier, the world box through a tree of divergent branches), and it re-reads a class scalar from the kernel-argument
// segment rather than keep it in a register -- with a wait on the counter the LDS reads share, in the middle of those reads.  The empty
// statement takes the pointers as scalar-register inputs (they must be there at this point; they stay what they are to the optimiser)
// and hands the class scalars, the row offsets' pointer and the boxes' back as values of unknown origin: nothing behind it can be read
// again from the segment.
// (kmax, max_steps, cacheC, x_init, x_out, obj_out, status_out and info_out are first read behind the first pass, and every use reads them
// from the segment again.  Listed here they cost a second wait and twelve lane spills in front of the first load of the critical chain;
// without them that block is 19 instructions shorter and the stepping instance 120 cycles SLOWER in the timing twin -- the reads then
// stand, with waits of their own, in front of the loop of steps: NOTES section 45.  They stay listed.)
// (a pointer of unknown origin is a generic one, and a load through it waits on both counters: these two say "global memory" themselves)
#define LSCQP_DAS_GLOBAL __attribute__((address_space(1)))
#define LSCQP_DAS_KERNARGS()                                                                                                            \
    double ka_wb0 = cls.world_min[0], ka_wb1 = cls.world_min[1], ka_wb2 = cls.world_min[2];                                            \
    double ka_wb3 = cls.world_max[0], ka_wb4 = cls.world_max[1], ka_wb5 = cls.world_max[2];                                            \
    double ka_dt = cls.dt, ka_q2s = cls.q2s, ka_w_t = cls.w_t, ka_w_c = cls.w_c, ka_comm_range = cls.comm_range;                               \
    int ka_use_sfc = cls.use_sfc, ka_rsfc = cls.rsfc;                                                                                  \
    const int32_t* const ka_order = cls.order;                                                                                        \
    LSCQP_DAS_GLOBAL const uint64_t* ka_roffs = (LSCQP_DAS_GLOBAL const uint64_t*)row_offsets;                                         \
    LSCQP_DAS_GLOBAL const double* ka_sfc = (LSCQP_DAS_GLOBAL const double*)sfc;                                                       \
    asm volatile(""                                                                                                                    \
                 : "+s"(ka_wb0), "+s"(ka_wb1), "+s"(ka_wb2), "+s"(ka_wb3), "+s"(ka_wb4), "+s"(ka_wb5), "+s"(ka_dt), "+s"(ka_q2s),      \
                   "+s"(ka_w_t), "+s"(ka_w_c), "+s"(ka_comm_range), "+s"(ka_use_sfc), "+s"(ka_rsfc), "+s"(ka_roffs), "+s"(ka_sfc)                   \
                 : "s"(ka_order), "s"(tab), "s"(hdr), "s"(rows), "s"(n), "s"(cap), "s"(kmax), "s"(max_steps),        \
                   "s"(cacheC), "s"(stage_rows), "s"(x_init), "s"(x_out), "s"(obj_out), "s"(status_out), "s"(info_out))

// One row of the model as (<= 3 entries, right-hand side): a'c >= h.  An entry names (axis, control point) as axis << 16 | cp.
struct Row {
    int ent[3];
    double coef[3];
    double rhs;
};
__device__ __forceinline__ int ent_axis(int e) { return e >> 16; }
__device__ __forceinline__ int ent_cp(int e) { return e & 0xffff; }

// C couples control points of the same axis only.
// (C a)[axis kx, control point cp]
__device__ __forceinline__ double ccol(const int* ea, const double* ca, int kx, int cp, const double* __restrict__ Cm, int P) {
    // (loads without a test -- an unused entry is (axis 0, control point 0) with coefficient 0 -- so that the three are in flight together)
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double v = Cm[(size_t)ent_cp(ea[i]) * P + cp];
        s += ((ent_axis(ea[i]) == kx) ? ca[i] : 0.0) * v;
    }
    return s;
}
// a'C b for two rows
__device__ __forceinline__ double cdot(const int* ea, const double* ca, const int* eb, const double* cb, const double* __restrict__ Cm, int P) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double v = Cm[(size_t)ent_cp(ea[i]) * P + ent_cp(eb[j])];
            s += ((ent_axis(ea[i]) == ent_axis(eb[j])) ? ca[i] * cb[j] : 0.0) * v;
        }
    }
    return s;
}

#ifndef LSCQP_DAS_KU1
#define LSCQP_DAS_KU1 2
#endif
#ifndef LSCQP_DAS_WPE1
#define LSCQP_DAS_WPE1 3
#endif
// SCREEN: the lean form for batches that fill the chip -- unconstrained minimiser, ONE pass over the rows, verification; an instance with a
// violated row is left (LSCQP_STATUS_ITER_LIMIT) to the full form, which runs behind it over the same batch and skips what is OPTIMAL
// (`behind` != 0).  Without the step loop the kernel needs half the registers: twice the wavefronts per SIMD for the phase that streams
// the rows from HBM.
#ifndef LSCQP_DAS_WPES
#define LSCQP_DAS_WPES 4
#endif
// What the phase did with its instance (the same in every thread of the workgroup).
enum DasVerdict { kDasSolved = 0, kDasInfeasible = 1, kDasHandedOver = 2 };  // solved: OPTIMAL, also one `behind` found OPTIMAL; handed over: ITER_LIMIT

template <int NW, bool F32, bool SCREEN = false, bool PEEL = false>
__global__ __launch_bounds__(64 * NW, (SCREEN ? LSCQP_DAS_WPES : NW == 1 ? LSCQP_DAS_WPE1 : 1)) void das_kernel(DevClass cls, int M, int dim, int es, int cap, int kmax, int max_steps, int cacheC, int stage_rows, int behind,
                                                      const double* __restrict__ tab, int64_t n, const lscqp_header* __restrict__ hdr,
                                                      const lscqp_row* __restrict__ rows, const uint64_t* __restrict__ row_offsets,
                                                      const lscqp_box* __restrict__ sfc, const double* __restrict__ x_init, double* __restrict__ x_out,
                                                      double* __restrict__ obj_out, int32_t* __restrict__ status_out, lscqp_info* __restrict__ info_out) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int T = 64 * NW;
    constexpr int kU = SCREEN ? 4 : (NW == 1) ? LSCQP_DAS_KU1 : 4;  // LSC rows in flight per thread (the one-wavefront full form trades them for a third wavefront per SIMD)
    constexpr int kMaxNL = 0x7fffffff;  // (LSC rows per instance: bounded by `cap` at run time only)
    const int64_t k0 = blockIdx.x;
    if (k0 >= n) return;
    const int64_t q = cls.order ? (int64_t)cls.order[k0] : k0;
    // (the throughput text: with the kernel-argument block every one-wavefront form moved in vector registers, and three forms spilled more
    // scalar registers -- NOTES section 23; these forms run the batches that fill the chip, where a quiet instance must not pay for step setup)
#define LSCQP_DAS_FORM LSCQP_DAS_THROUGHPUT
#define LSCQP_DAS_END(verdict_) return
#include "lscqp_das_body.inc"
#undef LSCQP_DAS_END
#undef LSCQP_DAS_FORM
}

}  // namespace lscqp_das

