// lscqp_prescreen.hip — the PRESCREEN: per-control-point infeasibility, proven in one pass in front of the dual active-set phase
// (include/lscqp.h, "prescreen").  gfx950, one wavefront per instance, one lane per control point (m, i), looping where 6 M > 64.
//
// Why: an LSC row (src/traj_optimizer.cpp:413-429), a corridor face (:372-397) and a world face (:252-253) each touch ONE control point.  If
// the rows of one control point have no common point, the QP has none -- the reference gets that verdict from CPLEX's presolve and falls back
// at once (src/traj_optimizer.cpp:103-144, src/traj_planner.cpp:767-797), the dual active-set phase needs ~70 steps for it.  In three
// variables an empty row system has an empty subsystem of at most four rows (Helly), so the test is small, exact and independent per lane.
//
// The test of one control point (test_point): Goldfarb-Idnani on "the point nearest to the interval's centre", three variables, at most
// `dim` active rows, everything in registers; the rows are re-read (L2) in every step, `[obstacle][m][i]` order, so consecutive lanes read
// consecutive rows.  The search runs on the rows RELAXED by kRelax (3e-6 m): a control point whose rows are empty by 1e-5 m or more ends in
// the method's stopping case -- a violated row whose normal lies in the cone of the active ones, no multiplier gives way -- whatever the
// rounding of a step does.  That case yields lambda >= 0, sum 1, over at most dim + 1 rows.
// What is FIRED is checked on the ORIGINAL rows, normalised (n^, b^ = (b - n.p0) / |n|, coordinates relative to the agent's position):
//     rho = sum lambda_i n^_i,  v = sum lambda_i b^_i,  D = the largest distance from p0 to a corner of the world box (the class's `dim` axes),
//     proven violation = v - |rho|_1 D >= 1e-6 m  (the figure of the phase's own proof)
// -- every point c of the world box has |c_k - p0_k| <= D, so sum lambda_i (b^_i - n^_i.c) >= v - |rho|_1 D there: some row is violated by that
// much at every point.  No tolerance of the search can produce a false verdict; a doubtful control point does not fire, nor does one whose
// search runs out of its step budget, and the solver decides the instance as without the prescreen.
//
// Not tested: the three fixed control points of segment 0 -- the reference adds no LSC row there (:404-406) and the solver drops them, so a
// row violated at c0, c1 or c2 proves nothing about the QP; the interval holds the single-variable rows (world box, corridor,
// the waypoint's communication range on c[m][5]) and not the communication rows that tie c[m][5] to another control point (the row-for-row
// model writes those against c[mi][0]: leaving them out makes the interval wider, never tighter); RSFC classes
// (z of segment 0 is bounded by +-100, not the world box: D would not cover it).  No scratch, no atomics, no LDS, no waiting across workgroups.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "lscqp_kernel.hpp"
#include "lscqp_internal.hpp"

namespace lscqp_pre {

constexpr double kBar = 1e-6;     // proven violation a fired control point carries at least (metres)
constexpr double kBarRounding = 1e-11;  // ... plus this much for the rounding of the check itself (terms of ~10 m in fp64: ~1e-14)
constexpr double kRelax = 3e-6;   // the search's relaxation of every row: between the bar and the 1e-5 m from which a control point MUST fire
constexpr double kViolated = 1e-9;  // a relaxed row counts as violated below this slack
constexpr int kSteps = 48;        // steps (rows added + rows dropped) of one control point's search; beyond: not fired

struct PointCert {  // (scalars, not arrays: nothing here may end up in scratch memory)
    int n_rows;
    int r0, r1, r2, r3;
    double w0, w1, w2, w3;
    double viol;
};

template <bool F32>
__host__ __device__ __forceinline__ void fetch_row(const void* rows, uint64_t idx, double& x, double& y, double& z, double& w) {
    if constexpr (F32) {
        const float4 f = reinterpret_cast<const float4*>(rows)[idx];
        x = f.x, y = f.y, z = f.z, w = f.w;
    } else {
        const double4 d = reinterpret_cast<const double4*>(rows)[idx];
        x = d.x, y = d.y, z = d.z, w = d.w;
    }
}

// row `id` of control point cp, normalised and relative to the agent's position: n^.c >= b^.  id >= 0: the LSC row of obstacle id (false: the
// solver drops it, :409-411, or it has no part in the class's axes); id = -1 - (2 axis + side): an interval face, side 0 = lower
template <bool F32>
__host__ __device__ __forceinline__ bool unit_row(const void* rows, uint64_t roff, int P, int cp, int dim, int id, double o0, double o1, double o2,
                                                 double l0, double l1, double l2, double h0, double h1, double h2, double& nx, double& ny,
                                                 double& nz, double& b) {
    if (id < 0) {
        const int f = -1 - id, k = f >> 1, side = f & 1;
        const double sg = side ? -1.0 : 1.0;
        nx = k == 0 ? sg : 0.0, ny = k == 1 ? sg : 0.0, nz = k == 2 ? sg : 0.0;
        const double lo = k == 0 ? l0 : k == 1 ? l1 : l2, hi = k == 0 ? h0 : k == 1 ? h1 : h2;
        b = side ? -hi : lo;
        return true;
    }
    double x, y, z, w;
    fetch_row<F32>(rows, roff + (uint64_t)id * (uint64_t)P + (uint64_t)cp, x, y, z, w);
    const bool dropped = x * x + y * y + z * z < 1e-10;  // (as the phase: |n| < 1e-5)
    if (dim != 3) z = 0.0;
    const double nn = sqrt(x * x + y * y + z * z);
    const double inv = nn > 0.0 ? 1.0 / nn : 0.0;
    nx = x * inv, ny = y * inv, nz = z * inv;
    b = (w - (x * o0 + y * o1 + z * o2)) * inv;
    return !dropped && nn > 0.0;
}

// One free control point: do its rows have a common point?  true: NO, with the checked certificate in `out`.
template <bool F32>
__host__ __device__ __forceinline__ bool test_point(const void* rows, uint64_t roff, int n_obs, int P, int cp, int dim, double o0, double o1, double o2, double l0,
                                           double l1, double l2, double h0, double h1, double h2, double D, PointCert& out) {
    auto row = [&](int id, double& nx, double& ny, double& nz, double& b) -> bool {
        return unit_row<F32>(rows, roff, P, cp, dim, id, o0, o1, o2, l0, l1, l2, h0, h1, h2, nx, ny, nz, b);
    };
    // the point, from the interval's centre (axes the class does not have stay 0: no row has a part there)
    double x0 = 0.5 * (l0 + h0), x1 = 0.5 * (l1 + h1), x2 = dim == 3 ? 0.5 * (l2 + h2) : 0.0;
    // active rows: three slots (a free slot holds a zero normal, multiplier 0 and a unit diagonal in the Gram matrix below)
    bool act[3] = {false, false, false};
    int aid[3] = {0, 0, 0};
    double an[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, ab[3] = {0, 0, 0}, au[3] = {0, 0, 0};
    int nact = 0;
    bool have = false;  // a candidate row is being worked in (kept across partial steps)
    int pid = 0;
    double p0 = 0, p1 = 0, p2 = 0, pb = 0, pu = 0;
    for (int step = 0; step < kSteps; step++) {
        if (!have) {  // the most violated relaxed row at the point, lowest id on ties: faces first (ids < 0, descending), then LSC rows
            double worst = -kViolated;
            for (int f = 0; f < 2 * dim; f++) {
                double nx, ny, nz, b;
                (void)row(-1 - f, nx, ny, nz, b);
                const double s = nx * x0 + ny * x1 + nz * x2 - (b - kRelax);
                if (s < worst) worst = s, have = true, pid = -1 - f, p0 = nx, p1 = ny, p2 = nz, pb = b;
            }
            for (int o = 0; o < n_obs; o++) {
                double nx, ny, nz, b;
                const bool used = row(o, nx, ny, nz, b);
                const double s = nx * x0 + ny * x1 + nz * x2 - (b - kRelax);
                if (used && s < worst) worst = s, have = true, pid = o, p0 = nx, p1 = ny, p2 = nz, pb = b;
            }
            if (!have) return false;  // a point of the relaxed rows: nothing to prove
            pu = 0.0;
        }
        // r = (A'A)^-1 A'p over the active rows, z = p - A r: the step direction in the point, -r in the multipliers
        const double d0 = an[0][0] * p0 + an[0][1] * p1 + an[0][2] * p2, d1 = an[1][0] * p0 + an[1][1] * p1 + an[1][2] * p2,
                     d2 = an[2][0] * p0 + an[2][1] * p1 + an[2][2] * p2;
        const double g00 = 1.0, g11 = 1.0, g22 = 1.0;  // (unit rows; a free slot's diagonal is 1 as well, its off-diagonals 0)
        const double g01 = an[0][0] * an[1][0] + an[0][1] * an[1][1] + an[0][2] * an[1][2];
        const double g02 = an[0][0] * an[2][0] + an[0][1] * an[2][1] + an[0][2] * an[2][2];
        const double g12 = an[1][0] * an[2][0] + an[1][1] * an[2][1] + an[1][2] * an[2][2];
        const double c00 = g11 * g22 - g12 * g12, c01 = g02 * g12 - g01 * g22, c02 = g01 * g12 - g02 * g11;
        const double c11 = g00 * g22 - g02 * g02, c12 = g01 * g02 - g00 * g12, c22 = g00 * g11 - g01 * g01;
        const double det = g00 * c00 + g01 * c01 + g02 * c02;
        if (!(det > 1e-14)) return false;  // dependent active rows: not ours to judge
        const double idet = 1.0 / det;
        double r[3];
        r[0] = (c00 * d0 + c01 * d1 + c02 * d2) * idet;
        r[1] = (c01 * d0 + c11 * d1 + c12 * d2) * idet;
        r[2] = (c02 * d0 + c12 * d1 + c22 * d2) * idet;
        double z0 = p0 - (r[0] * an[0][0] + r[1] * an[1][0] + r[2] * an[2][0]);
        double z1 = p1 - (r[0] * an[0][1] + r[1] * an[1][1] + r[2] * an[2][1]);
        double z2 = p2 - (r[0] * an[0][2] + r[1] * an[1][2] + r[2] * an[2][2]);
        const bool full = nact >= dim;  // the active normals span the space: no direction is left
        if (full) z0 = z1 = z2 = 0.0;
        const double zz = z0 * z0 + z1 * z1 + z2 * z2;
        // the multiplier that gives way first
        double t1 = INFINITY;
        int jdrop = -1;
#pragma unroll
        for (int i = 0; i < 3; i++)
            if (act[i] && r[i] > 1e-12) {
                const double t = au[i] / r[i];
                if (t < t1) t1 = t, jdrop = i;
            }
        if (jdrop < 0) {
            // none does.  The candidate and the active rows with weights (1, -r), scaled to sum 1, are a certificate if the part of the
            // candidate's normal outside their cone is small enough: checked here, on the unrelaxed rows, with rho as it comes out
            double lm0 = act[0] ? fmax(-r[0], 0.0) : 0.0, lm1 = act[1] ? fmax(-r[1], 0.0) : 0.0, lm2 = act[2] ? fmax(-r[2], 0.0) : 0.0;
            const double is = 1.0 / (1.0 + lm0 + lm1 + lm2);
            lm0 *= is, lm1 *= is, lm2 *= is;
            const double rx = is * p0 + lm0 * an[0][0] + lm1 * an[1][0] + lm2 * an[2][0], ry = is * p1 + lm0 * an[0][1] + lm1 * an[1][1] + lm2 * an[2][1],
                         rz = is * p2 + lm0 * an[0][2] + lm1 * an[1][2] + lm2 * an[2][2];
            const double v = is * pb + lm0 * ab[0] + lm1 * ab[1] + lm2 * ab[2];
            const double proven = v - (fabs(rx) + fabs(ry) + fabs(rz)) * D;
            if (proven >= kBar + kBarRounding) {
                // the candidate first, then the active rows that carry weight (selects on the count, not an indexed store)
                int k = 1;
                out.r0 = pid, out.w0 = is;
                out.r1 = out.r2 = out.r3 = 0;
                out.w1 = out.w2 = out.w3 = 0.0;
                auto put = [&](int id, double l) {
                    out.r1 = k == 1 ? id : out.r1, out.w1 = k == 1 ? l : out.w1;
                    out.r2 = k == 2 ? id : out.r2, out.w2 = k == 2 ? l : out.w2;
                    out.r3 = k == 3 ? id : out.r3, out.w3 = k == 3 ? l : out.w3;
                    k++;
                };
                if (act[0] && lm0 > 0.0) put(aid[0], lm0);
                if (act[1] && lm1 > 0.0) put(aid[1], lm1);
                if (act[2] && lm2 > 0.0) put(aid[2], lm2);
                out.n_rows = k;
                out.viol = proven;
                return true;
            }
            if (full || !(zz > 1e-20)) return false;  // no step either: doubtful, left to the solver
        }
        const double slack = (pb - kRelax) - (p0 * x0 + p1 * x1 + p2 * x2);  // > 0: what the candidate still lacks
        const double t2 = (!full && zz > 1e-20) ? slack / zz : INFINITY;
        const bool partial = t1 < t2;
        const double t = partial ? t1 : t2;
        x0 += t * z0, x1 += t * z1, x2 += t * z2;
        pu += t;
#pragma unroll
        for (int i = 0; i < 3; i++)
            if (act[i]) au[i] = fmax(au[i] - t * r[i], 0.0);
        if (partial) {  // the blocking row leaves; the candidate stays
#pragma unroll
            for (int i = 0; i < 3; i++)
                if (i == jdrop) act[i] = false, an[i][0] = an[i][1] = an[i][2] = 0.0, ab[i] = 0.0, au[i] = 0.0;
            nact--;
        } else {  // the candidate is met: it joins the active rows in the first free slot
            bool placed = false;
#pragma unroll
            for (int i = 0; i < 3; i++)
                if (!placed && !act[i]) {
                    placed = true;
                    act[i] = true, aid[i] = pid, an[i][0] = p0, an[i][1] = p1, an[i][2] = p2, ab[i] = pb, au[i] = pu;
                }
            nact++;
            have = false;
        }
    }
    return false;  // out of steps
}

// the interval of control point cp = 6 m + i (world box, corridor of its segment, and on c[m][5] the communication range about the next
// waypoint, :492-498 -- every single-variable row of the model), relative to the agent's position, and D
__host__ __device__ __forceinline__ void interval_of(const lscqp::DevClass& cls, int dim, const lscqp_box* sfc_q, const lscqp_header* Hd, int cp, double o0, double o1, double o2,
                                                    double& l0, double& l1, double& l2, double& h0, double& h1, double& h2, double& D) {
    l0 = cls.world_min[0], l1 = cls.world_min[1], l2 = cls.world_min[2];
    h0 = cls.world_max[0], h1 = cls.world_max[1], h2 = cls.world_max[2];
    const double e0 = fmax(fabs(l0 - o0), fabs(h0 - o0)), e1 = fmax(fabs(l1 - o1), fabs(h1 - o1)), e2 = dim == 3 ? fmax(fabs(l2 - o2), fabs(h2 - o2)) : 0.0;
    D = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
    if (cls.use_sfc) {  // (uniform) :372-397
        const lscqp_box bx = sfc_q[cp / 6];
        l0 = fmax(l0, bx.bmin[0]), l1 = fmax(l1, bx.bmin[1]), l2 = fmax(l2, bx.bmin[2]);
        h0 = fmin(h0, bx.bmax[0]), h1 = fmin(h1, bx.bmax[1]), h2 = fmin(h2, bx.bmax[2]);
    }
    if (cls.comm_range > 0 && cp % 6 == 5) {  // :492-498
        const double rw = 0.5 * cls.comm_range - 1e-5;
        const double w0 = Hd->next_waypoint[0], w1 = Hd->next_waypoint[1], w2 = Hd->next_waypoint[2];
        l0 = fmax(l0, w0 - rw), l1 = fmax(l1, w1 - rw), l2 = fmax(l2, w2 - rw);
        h0 = fmin(h0, rw + w0), h1 = fmin(h1, rw + w1), h2 = fmin(h2, rw + w2);
    }
    l0 -= o0, l1 -= o1, l2 -= o2, h0 -= o0, h1 -= o1, h2 -= o2;
}

__host__ __device__ __forceinline__ bool judged(const lscqp::DevClass& cls, int n_obs, int cap) { return n_obs >= 0 && n_obs <= cap && !cls.rsfc; }

// One wavefront per instance.  cert_out != NULL: the standalone entry, one certificate per instance and nothing else.  status_out != NULL: in
// front of a solve -- a fired instance gets what the phase's own verdict writes (lscqp_das_body.inc, infeasible_out) with
// LSCQP_INFO_PRESCREENED beside LSCQP_INFO_ACTIVE_SET, every other one LSCQP_STATUS_ITER_LIMIT ("nobody has solved it yet").
// (four wavefronts per SIMD: the compiler's own choice was 130 VGPRs, three wavefronts; held to 128 it spills nothing -- 127 VGPRs, no scratch)
template <bool F32>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void prescreen_kernel(lscqp::DevClass cls, int M, int dim, int cap, int64_t n, const lscqp_header* __restrict__ hdr,
                                                       const void* __restrict__ rows, const uint64_t* __restrict__ row_offsets,
                                                       const lscqp_box* __restrict__ sfc, const double* __restrict__ x_init,
                                                       lscqp_prescreen_cert* __restrict__ cert_out, double* __restrict__ x_out,
                                                       double* __restrict__ obj_out, int32_t* __restrict__ status_out, lscqp_info* __restrict__ info_out) {
    const int64_t q = blockIdx.x;
    if (q >= n) return;
    const int lane = threadIdx.x;
    const int P = 6 * M, NX = dim * P;
    const lscqp_header* Hd = hdr + q;
    const int n_obs = Hd->n_obs;
    const double o0 = Hd->p0[0], o1 = Hd->p0[1], o2 = Hd->p0[2];
    const uint64_t roff = row_offsets ? row_offsets[q] : 0;
    const bool ok = judged(cls, n_obs, cap);  // (uniform)
    int win_cp = -1;
    PointCert pc;
    pc.n_rows = 0, pc.viol = 0.0;
    pc.r0 = pc.r1 = pc.r2 = pc.r3 = 0;
    pc.w0 = pc.w1 = pc.w2 = pc.w3 = 0.0;
    if (ok && n_obs > 0 && rows) {
        for (int base = 0; base < P; base += 64) {  // (uniform)
            const int cp = base + lane;
            const int cpc = cp < P ? cp : P - 1;  // (clamped: every address a lane forms lies inside the instance's rows)
            double l0, l1, l2, h0, h1, h2, D;
            interval_of(cls, dim, sfc + q * M, Hd, cpc, o0, o1, o2, l0, l1, l2, h0, h1, h2, D);
            bool fired = false;
            if (cp < P && cp >= 3) fired = test_point<F32>(rows, roff, n_obs, P, cpc, dim, o0, o1, o2, l0, l1, l2, h0, h1, h2, D, pc);
            const unsigned long long mask = __ballot(fired);
            if (mask) {  // (uniform) the lowest firing control point of the instance: its lane's certificate to every lane
                const int w = __ffsll((long long)mask) - 1;
                win_cp = base + w;
                pc.n_rows = __shfl(pc.n_rows, w);
                pc.viol = __shfl(pc.viol, w);
                pc.r0 = __shfl(pc.r0, w), pc.r1 = __shfl(pc.r1, w), pc.r2 = __shfl(pc.r2, w), pc.r3 = __shfl(pc.r3, w);
                pc.w0 = __shfl(pc.w0, w), pc.w1 = __shfl(pc.w1, w), pc.w2 = __shfl(pc.w2, w), pc.w3 = __shfl(pc.w3, w);
                break;
            }
        }
    }
    const bool fired = win_cp >= 0;
    if (cert_out && lane == 0) {
        lscqp_prescreen_cert c;
        c.fired = fired ? 1 : 0;
        c.control_point = win_cp;
        c.n_rows = fired ? pc.n_rows : 0;
        c.reserved = 0;
        auto rid = [&](int i, int id) { return (fired && i < pc.n_rows) ? (id >= 0 ? id * P + win_cp : id) : 0; };  // (an LSC row by its index in the instance's row list)
        auto wgt = [&](int i, double l) { return (fired && i < pc.n_rows) ? l : 0.0; };
        c.row[0] = rid(0, pc.r0), c.row[1] = rid(1, pc.r1), c.row[2] = rid(2, pc.r2), c.row[3] = rid(3, pc.r3);
        c.lambda[0] = wgt(0, pc.w0), c.lambda[1] = wgt(1, pc.w1), c.lambda[2] = wgt(2, pc.w2), c.lambda[3] = wgt(3, pc.w3);
        c.violation = fired ? pc.viol : 0.0;
        cert_out[q] = c;
    }
    if (status_out) {
        if (fired) {
            for (int e = lane; e < NX; e += 64) x_out[q * NX + e] = x_init ? x_init[q * NX + e] : Hd->p0[e / P];
            if (lane == 0) {
                obj_out[q] = 0.0;
                status_out[q] = LSCQP_STATUS_INFEASIBLE;
                if (info_out) {
                    info_out[q].iterations = 0;
                    info_out[q].flags = LSCQP_INFO_ACTIVE_SET | LSCQP_INFO_PRESCREENED;
                    info_out[q].res_primal = pc.viol;
                    info_out[q].res_dual = 0.0;
                    info_out[q].gap = 0.0;
                }
            }
        } else if (lane == 0) {
            status_out[q] = LSCQP_STATUS_ITER_LIMIT;
        }
    }
}

}  // namespace lscqp_pre

extern "C" hipError_t lscqp_launch_prescreen(const lscqp::DevClass* cls, int M, int dim, int cap, int64_t n, const lscqp_header* hdr, const lscqp_row* rows,
                                             const uint64_t* row_offsets, const lscqp_box* sfc, const double* x_init, lscqp_prescreen_cert* cert_out,
                                             double* x_out, double* obj_out, int32_t* status_out, lscqp_info* info_out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (cls->rows_f32)
        hipLaunchKernelGGL((lscqp_pre::prescreen_kernel<true>), dim3((unsigned)n), dim3(64), 0, stream, *cls, M, dim, cap, n, hdr, (const void*)rows,
                           row_offsets, sfc, x_init, cert_out, x_out, obj_out, status_out, info_out);
    else
        hipLaunchKernelGGL((lscqp_pre::prescreen_kernel<false>), dim3((unsigned)n), dim3(64), 0, stream, *cls, M, dim, cap, n, hdr, (const void*)rows,
                           row_offsets, sfc, x_init, cert_out, x_out, obj_out, status_out, info_out);
    return hipGetLastError();
}

extern "C" int lscqp_prescreen_host_twin_(const lscqp::DevClass* cls, int M, int dim, int cap, int64_t n, const lscqp_header* hdr, const void* rows,
                                          const uint64_t* row_offsets, const lscqp_box* sfc, lscqp_prescreen_cert* cert_out) {
    using namespace lscqp_pre;
    const int P = 6 * M;
    for (int64_t q = 0; q < n; q++) {
        lscqp_prescreen_cert c = {};
        c.control_point = -1;
        const int n_obs = hdr[q].n_obs;
        const double o0 = hdr[q].p0[0], o1 = hdr[q].p0[1], o2 = hdr[q].p0[2];
        const uint64_t roff = row_offsets ? row_offsets[q] : 0;
        if (judged(*cls, n_obs, cap) && n_obs > 0 && rows) {
            for (int cp = 3; cp < P && !c.fired; cp++) {
                double l0, l1, l2, h0, h1, h2, D;
                interval_of(*cls, dim, sfc + q * M, hdr + q, cp, o0, o1, o2, l0, l1, l2, h0, h1, h2, D);
                PointCert pc = {};
                const bool f = cls->rows_f32 ? test_point<true>(rows, roff, n_obs, P, cp, dim, o0, o1, o2, l0, l1, l2, h0, h1, h2, D, pc)
                                             : test_point<false>(rows, roff, n_obs, P, cp, dim, o0, o1, o2, l0, l1, l2, h0, h1, h2, D, pc);
                if (f) {
                    c.fired = 1, c.control_point = cp, c.n_rows = pc.n_rows, c.violation = pc.viol;
                    const int ids[4] = {pc.r0, pc.r1, pc.r2, pc.r3};
                    const double ws[4] = {pc.w0, pc.w1, pc.w2, pc.w3};
                    for (int i = 0; i < pc.n_rows; i++) c.row[i] = ids[i] >= 0 ? ids[i] * P + cp : ids[i], c.lambda[i] = ws[i];
                }
            }
        }
        cert_out[q] = c;
    }
    return 0;
}
