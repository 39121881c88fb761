// lscqp_das.hip — the DUAL ACTIVE SET phase of the batched trajectory-QP solver: its host side (tables, launch) and the kernel's
// instances.  The algorithm and the device code: lscqp_das.hpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <cmath>
#include <mutex>
#include <vector>

#include "lscqp_internal.hpp"
#include "lscqp_das.hpp"

// ---- host side ------------------------------------------------------------------------------------------------------------------------

// The tables of a class: for ts = 1 .. M  [U1 | U2 | G1 | C], C = T (T'Hx T)^-1 T' in extended precision (cond(T'Hx T) ~ 2e5 .. 3e6).
// Returns the number of doubles written (M * table_stride(M)); out may be NULL to ask for the size.
// The two-sided rows of a class, as far as they do not depend on the instance (the order and the ids of the kernel's table: intervals, velocity
// rows, acceleration rows, communication pairs): per row two ints -- the packed stencil the kernel keeps in LDS (type << 24 | e0 << 12 | e1)
// and what its bounds depend on (family | axis << 2 | segment << 4 | last control point of its segment << 8 | axis 2 of segment 0 << 9).
// The kernel reads them from behind the tables and the objective's rounding term instead of deriving them thread by thread with one
// branch per family.  Returns the number of rows (num_pairs); out == NULL: only that.
extern "C" size_t lscqp_das_build_pairs(int M, int dim, int comm_on, int32_t* out) {
    const int P = 6 * M, NX = dim * P, NCP = M * (M - 1) / 2;
    const int oV = NX, oA = oV + dim * 5 * M, oC = oA + dim * 4 * M, NPAIR = lscqp_das::num_pairs(M, dim);
    if (!out) return (size_t)NPAIR;
    for (int r = 0; r < NPAIR; r++) {
        int type = 0, e0 = 0, e1 = 0, fam = 0, k = 0, m = 0, last = 0;
        if (r < oV) {
            k = r / P;
            const int cp = r - k * P;
            m = cp / 6, last = cp % 6 == 5;
            type = cp >= 3 ? 1 : 0, e0 = r, fam = 0;
        } else if (r < oA) {
            const int s = r - oV;
            k = s / (5 * M);
            const int rr = s - k * 5 * M, i = rr % 5;
            m = rr / 5;
            type = (m == 0 && i < 2) ? 0 : 2, e0 = k * P + 6 * m + i, fam = 1;
        } else if (r < oC) {
            const int s = r - oA;
            k = s / (4 * M);
            const int rr = s - k * 4 * M, i = rr % 4;
            m = rr / 4;
            type = (m == 0 && i < 1) ? 0 : 3, e0 = k * P + 6 * m + i, fam = 2;
        } else {
            const int s = r - oC;
            k = s / NCP;
            const int ci = s - k * NCP;
            int uu = 1;
            while (uu * (uu + 1) / 2 <= ci) uu++;
            const int up = ci - uu * (uu - 1) / 2;
            type = comm_on ? 4 : 0, e0 = k * P + 6 * (up + 1), e1 = k * P + 6 * uu + 5, fam = 3, m = 0;
        }
        out[2 * r] = (type << 24) | (e0 << 12) | e1;
        out[2 * r + 1] = fam | (k << 2) | (m << 4) | (last << 8) | ((fam == 0 && k == 2 && m == 0) ? 1 << 9 : 0);
    }
    return (size_t)NPAIR;
}

extern "C" size_t lscqp_das_build_tables(int M, int es, double dt, double w_c, double w_t, double* out) {
    const int P = 6 * M, NZA = 3 * (M - 1) + (es ? 1 : 3);
    const size_t stride = lscqp_das::table_stride(M);
    if (!out) return stride * (size_t)M;
    typedef long double ld;
    const ld q2s = 2.0L * (ld)w_c / ((ld)dt * dt * dt * dt * dt);
    static const int kq[6][6] = {{720, -1800, 1200, 0, 0, -120},  {-1800, 4800, -3600, 0, 600, 0}, {1200, -3600, 3600, -1200, 0, 0},
                                 {0, 0, -1200, 3600, -3600, 1200}, {0, 600, 0, -3600, 4800, -1800}, {-120, 0, 0, 1200, -1800, 720}};
    static const int tbm[3][3] = {{0, 0, 1}, {0, -1, 2}, {1, -4, 4}};
    // T: P x NZA
    std::vector<ld> Tm((size_t)P * NZA, 0.0L);
    for (int m = 0; m < M; m++) {
        const bool last = es && m == M - 1;
        for (int j = 0; j < 3; j++) Tm[(size_t)(6 * m + 3 + j) * NZA + 3 * m + (last ? 0 : j)] = 1.0L;
        if (m >= 1)
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) Tm[(size_t)(6 * m + i) * NZA + 3 * (m - 1) + j] = (ld)tbm[i][j];
    }
    for (int ts = 1; ts <= M; ts++) {
        std::vector<ld> Hx((size_t)P * P, 0.0L);
        for (int m = 0; m < M; m++)
            for (int i = 0; i < 6; i++)
                for (int j = 0; j < 6; j++) Hx[(size_t)(6 * m + i) * P + 6 * m + j] += q2s * (ld)kq[i][j];
        for (int m = M - ts; m < M; m++) Hx[(size_t)(6 * m + 5) * P + 6 * m + 5] += 2.0L * (ld)w_t;
        // K0 = T'Hx T
        std::vector<ld> HT((size_t)P * NZA, 0.0L), K0((size_t)NZA * NZA, 0.0L);
        for (int i = 0; i < P; i++)
            for (int l = 0; l < P; l++) {
                const ld h = Hx[(size_t)i * P + l];
                if (h == 0.0L) continue;
                for (int j = 0; j < NZA; j++) HT[(size_t)i * NZA + j] += h * Tm[(size_t)l * NZA + j];
            }
        for (int i = 0; i < P; i++)
            for (int a = 0; a < NZA; a++) {
                const ld t = Tm[(size_t)i * NZA + a];
                if (t == 0.0L) continue;
                for (int b = 0; b < NZA; b++) K0[(size_t)a * NZA + b] += t * HT[(size_t)i * NZA + b];
            }
        // Cholesky K0 = R'R ... inverse through the factor
        std::vector<ld> Lc((size_t)NZA * NZA, 0.0L);
        for (int j = 0; j < NZA; j++) {
            ld d = K0[(size_t)j * NZA + j];
            for (int l = 0; l < j; l++) d -= Lc[(size_t)j * NZA + l] * Lc[(size_t)j * NZA + l];
            if (!(d > 0.0L)) return 0;  // (not SPD: the class has no active-set phase; cannot happen for w_c, w_t > 0)
            const ld dj = sqrtl(d);
            Lc[(size_t)j * NZA + j] = dj;
            for (int i = j + 1; i < NZA; i++) {
                ld s = K0[(size_t)i * NZA + j];
                for (int l = 0; l < j; l++) s -= Lc[(size_t)i * NZA + l] * Lc[(size_t)j * NZA + l];
                Lc[(size_t)i * NZA + j] = s / dj;
            }
        }
        // X = Lc^-1 T'  (NZA x P), C = X'X
        std::vector<ld> X((size_t)NZA * P, 0.0L);
        for (int col = 0; col < P; col++) {
            for (int i = 0; i < NZA; i++) {
                ld s = Tm[(size_t)col * NZA + i];
                for (int l = 0; l < i; l++) s -= Lc[(size_t)i * NZA + l] * X[(size_t)l * P + col];
                X[(size_t)i * P + col] = s / Lc[(size_t)i * NZA + i];
            }
        }
        double* const tb = out + (size_t)(ts - 1) * stride;
        std::vector<ld> Cm((size_t)P * P, 0.0L);
        for (int a = 0; a < P; a++)
            for (int b = 0; b <= a; b++) {
                ld s = 0.0L;
                for (int i = 0; i < NZA; i++) s += X[(size_t)i * P + a] * X[(size_t)i * P + b];
                Cm[(size_t)a * P + b] = Cm[(size_t)b * P + a] = s;
            }
        for (int e = 0; e < P; e++) {
            ld u1 = 0.0L, u2 = 0.0L, g1 = 0.0L;
            for (int i = 0; i < 6; i++) {
                u1 += Cm[(size_t)e * P + i] * q2s * (ld)kq[i][1];
                u2 += Cm[(size_t)e * P + i] * q2s * (ld)kq[i][2];
            }
            for (int m = M - ts; m < M; m++) g1 += Cm[(size_t)e * P + 6 * m + 5];
            tb[e] = (double)u1;
            tb[P + e] = (double)u2;
            tb[2 * P + e] = (double)g1;
        }
        for (size_t e = 0; e < (size_t)P * P; e++) tb[3 * P + e] = (double)Cm[e];
    }
    return stride * (size_t)M;
}

#ifdef LSCQP_DAS_TIMING
extern "C" int lscqp_das_cycles(unsigned long long* out, int reset) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(lscqp_das::das_cycles), sizeof(unsigned long long) * 16);
    if (reset) {
        unsigned long long z[16] = {0};
        (void)hipMemcpyToSymbol(HIP_SYMBOL(lscqp_das::das_cycles), z, sizeof z);
    }
    return 0;
}
#endif

extern "C" size_t lscqp_das_lds_bytes(int M, int dim, int kmax, int cacheC, int stage_rows) {
    return sizeof(double) * (size_t)lscqp_das::Layout::make(M, dim, kmax, cacheC, stage_rows).total;
}

// workgroups of the one-wavefront form a CU holds at once (registers and the LDS footprint of a launch with `kmax` active rows, no table
// copy, no staged rows), as the runtime computes it; 0 without a device
extern "C" int lscqp_das_blocks_per_cu(int M, int dim, int kmax, int rows_f32) {
    int nb = 0;
    const size_t lds = lscqp_das_lds_bytes(M, dim, kmax, 0, 0);
    const hipError_t e = rows_f32 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, lscqp_das::das_kernel<1, true, false, true>, 64, lds)
                                  : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, lscqp_das::das_kernel<1, false, false, true>, 64, lds);
    return e == hipSuccess ? nb : 0;
}

// Launch of the phase over a batch.  threads: 64, 128 or 256 per QP; kmax <= 32 active rows; stage_rows: LSC rows per instance kept in LDS
// after the first pass (0: re-read from L2 in every pass; an instance with more rows than that re-reads them too); cap: the obstacle
// capacity of the kernel instance that runs behind the phase (an instance beyond it is left to that kernel's LSCQP_STATUS_CAPACITY).
// screen bit 1: the first look inside the loop of steps (PEEL = false; four wavefronts only).  screen bit 0: the lean one-wavefront form first (unconstrained minimiser + one pass + verification at twice the occupancy), then the
// full form over what it left -- for batches that fill the chip, where most instances hold no active row at all.
// screen bit 2: the prescreen (lscqp_prescreen.hip) ran in front of this launch; instances it marked LSCQP_STATUS_INFEASIBLE are skipped.
extern "C" hipError_t lscqp_launch_das(const lscqp::DevClass* cls, int M, int dim, int es, int cap, int threads, int kmax, int max_steps, int cacheC,
                                       int stage_rows, int screen, const double* d_tab, int64_t n, const lscqp_header* hdr, const lscqp_row* rows,
                                       const uint64_t* row_offsets, const lscqp_box* sfc, const double* x_init, double* x_out, double* obj_out,
                                       int32_t* status_out, lscqp_info* info_out, hipStream_t stream) {
    if (kmax < 1 || kmax > lscqp_das::kMaxK || (threads != 64 && threads != 128 && threads != 256)) return hipErrorInvalidValue;
    const size_t lds = lscqp_das_lds_bytes(M, dim, kmax, cacheC, stage_rows);
    if (lds > lscqp::kMaxLdsBytes) return hipErrorInvalidValue;
    static std::atomic<bool> attr_set[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    if (!attr_set[dev].load(std::memory_order_acquire)) {
        for (const void* f : {reinterpret_cast<const void*>(lscqp_das::das_kernel<1, false, false, true>), reinterpret_cast<const void*>(lscqp_das::das_kernel<2, false, false, true>),
                              reinterpret_cast<const void*>(lscqp_das::das_kernel<4, false, false, true>), reinterpret_cast<const void*>(lscqp_das::das_kernel<1, true, false, true>),
                              reinterpret_cast<const void*>(lscqp_das::das_kernel<2, true, false, true>), reinterpret_cast<const void*>(lscqp_das::das_kernel<4, true, false, true>),
                              reinterpret_cast<const void*>(lscqp_das::das_kernel<4, false>), reinterpret_cast<const void*>(lscqp_das::das_kernel<4, true>),
                              reinterpret_cast<const void*>(lscqp_das::das_kernel<1, false, true>), reinterpret_cast<const void*>(lscqp_das::das_kernel<1, true, true>)}) {
            const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lscqp::kMaxLdsBytes);
            if (e != hipSuccess) return e;
        }
        attr_set[dev].store(true, std::memory_order_release);
    }
    if (n <= 0) return hipSuccess;
    const bool f32 = cls->rows_f32 != 0;
    int behind = (screen & 4) ? 2 : 0;  // (bit 1: the prescreen ran in front -- what it marked LSCQP_STATUS_INFEASIBLE is skipped)
    const bool loop_form = (screen & 2) != 0;  // (the first look inside the loop of steps: the four-wavefront form of small batches)
    if (screen & 1) {
        const size_t lds_s = lscqp_das_lds_bytes(M, dim, 1, 0, 0);  // (no active rows, no table copy, no staged rows)
#define LSCQP_DAS_SCREEN(F_)                                                                                                                                  \
    hipLaunchKernelGGL((lscqp_das::das_kernel<1, F_, true>), dim3((unsigned)n), dim3(64), lds_s, stream, *cls, M, dim, es, cap, 1, 0, 0, 0, 0, d_tab, n, hdr, rows, \
                       row_offsets, sfc, x_init, x_out, obj_out, status_out, info_out)
        if (f32) LSCQP_DAS_SCREEN(true); else LSCQP_DAS_SCREEN(false);
#undef LSCQP_DAS_SCREEN
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        behind |= 1;
    }
#define LSCQP_DAS_LAUNCH(NW_, F_, PEEL_)                                                                                                                       \
    hipLaunchKernelGGL((lscqp_das::das_kernel<NW_, F_, false, PEEL_>), dim3((unsigned)n), dim3(64 * NW_), lds, stream, *cls, M, dim, es, cap, kmax, max_steps, cacheC, \
                       stage_rows, behind, d_tab, n, hdr, rows, row_offsets, sfc, x_init, x_out, obj_out, status_out, info_out)
    if (threads == 64) { if (f32) LSCQP_DAS_LAUNCH(1, true, true); else LSCQP_DAS_LAUNCH(1, false, true); }
    else if (threads == 128) { if (f32) LSCQP_DAS_LAUNCH(2, true, true); else LSCQP_DAS_LAUNCH(2, false, true); }
    else if (!loop_form) { if (f32) LSCQP_DAS_LAUNCH(4, true, true); else LSCQP_DAS_LAUNCH(4, false, true); }
    else { if (f32) LSCQP_DAS_LAUNCH(4, true, false); else LSCQP_DAS_LAUNCH(4, false, false); }
#undef LSCQP_DAS_LAUNCH
    return hipGetLastError();
}
