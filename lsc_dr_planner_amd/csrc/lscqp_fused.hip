// The dual active-set phase and the first interior-point pass behind it in ONE launch, for batches of at most one instance per CU.
// Built like lscqp_inst.hip, once per instance of LSCQP_FUSED_INSTANCES (lscqp_launch.hpp), with -DLSCQP_M=<M> -DLSCQP_DIM=<dim>
// -DLSCQP_ES=<0|1> -DLSCQP_NSLOT=<slots> -DLSCQP_W=<wavefronts per QP>; exports lscqp_launch_fused_<M>_<dim>_<ES>_<NSLOT>_<W>.
//
// Why: behind the phase the pass usually finds nothing to do -- every workgroup loads one status, sees OPTIMAL and leaves -- and on a batch
// of 64 that near-empty launch was 9 - 12 % of the call (profiles/r06_*).  The device entries cannot skip it (the host learns nothing of the
// statuses before it enqueues), so here the workgroup that handed its instance over solves it itself, right behind the phase.
#include <atomic>

#include "lscqp_kernel.hpp"
#include "lscqp_launch.hpp"
// (last: its fp-contraction pragma holds to the end of this file -- lscqp_pdip_one above keeps the instances' own setting)
#define LSCQP_DAS_CYCLES das_fused_cycles  // (-DLSCQP_DAS_TIMING, tools/das_timing.py: beside lscqp_das.hip's own totals in one library)
#include "lscqp_das.hpp"

#define LSCQP_FCAT_(a, b, c, d, e, f) a##b##_##c##_##d##_##e##_##f
#define LSCQP_FCAT(a, b, c, d, e, f) LSCQP_FCAT_(a, b, c, d, e, f)
#define LSCQP_FUSED_FN LSCQP_FCAT(lscqp_launch_fused_, LSCQP_M, LSCQP_DIM, LSCQP_ES, LSCQP_NSLOT, LSCQP_W)

namespace lscqp_das {

// The phase's LDS carve of a fused instance, fixed at compile time: the class's shape, the table copy, room for the staged rows of
// MAX_OBS obstacles, and 32 active rows -- or 20 where 32 would not fit beside those (M = 10 in 3-D, MAX_OBS = 40).  Every LDS offset of
// the phase is then an immediate.  A launch asks for budgets at or below these capacities; one that asks for more is refused (two
// launches).  The host gives a batch of at most one instance per CU 32 active rows whenever they fit beside ITS staged rows and the table
// (lscqp_api.hip): for the M = 10, 3-D instance that is a batch of at most 30 obstacles, which this carve therefore refuses -- such a batch
// runs the two launches of the parent form (NOTES.md section 16); the configs[3] shard (40 obstacles) gets 20 from the host and is fused.
constexpr bool carve_fits(int M, int dim, int kmax, int stage_rows) {
    return sizeof(double) * (size_t)Layout::make(M, dim, kmax, 1, stage_rows).total <= lscqp::kMaxLdsBytes;
}
// Which of the phase's two texts runs here (lscqp_das_body.inc, LSCQP_DAS_FORM; its header says what the latency text does differently):
// the M = 5 form and the M = 10, 2-D form run the latency text, with which they spill 150 and 196 scalar registers (their units are
// built without machine-level hoisting -- build.py: fused_flags, NOTES section 45; 161 and 220 with it).  The rule of NOTES
// section 24 decided per form: a change stays where the scalar-register spills do not grow or a timing pays for the growth.  Any other
// shape -- the M = 10, 3-D form -- keeps the throughput text: there the kernel-argument block costs scalar registers (306 SGPR spills
// against 292), and so did the first-step setup ahead of the first step (301 - 312 against 292); it has not been built with the rest.
// (this unit is compiled once per instance: the shape is the preprocessor's as well as the template's)
#if LSCQP_M == 5 || (LSCQP_M == 10 && LSCQP_DIM == 2)
#define LSCQP_DAS_FORM LSCQP_DAS_LATENCY
#else
#define LSCQP_DAS_FORM LSCQP_DAS_THROUGHPUT
#endif
template <int M, int DIM, bool ES, int NSLOT, int W>
struct FusedCarve {
    static constexpr int kStage = lscqp::Cfg<M, DIM, ES, NSLOT, W, (int)sizeof(double)>::MAX_OBS * 6 * M;  // LSC rows of a full instance
    static constexpr int KMAX = carve_fits(M, DIM, kMaxK, kStage) ? kMaxK : 20;
    static_assert(carve_fits(M, DIM, KMAX, kStage), "the fused phase's carve does not fit the CU's LDS");
};

// One workgroup of four wavefronts per instance: the phase's small-batch form (das_kernel<4, false, false, false>), then -- for an instance
// it handed over -- the first W wavefronts run the interior-point instance on it with cls.repair = 3, exactly as the separate launch would.
template <int M, int DIM, bool ES, int NSLOT, int W>
__global__ __launch_bounds__(256, 1) void das_pdip_kernel(DevClass cls, int cap, int kmax, int max_steps, int cacheC, int stage_rows,
                                                          const double* __restrict__ tab, int64_t n, const lscqp_header* __restrict__ hdr,
                                                          const lscqp_row* __restrict__ rows, const uint64_t* __restrict__ row_offsets,
                                                          const lscqp_box* __restrict__ sfc, const double* __restrict__ x_init,
                                                          double* __restrict__ x_out, double* __restrict__ obj_out, int32_t* __restrict__ status_out,
                                                          lscqp_info* __restrict__ info_out) {
    static_assert(W >= 1 && W <= 4, "the interior-point instance runs on the first W of the workgroup's four wavefronts");
    extern __shared__ __attribute__((aligned(16))) double smem[];
#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
    LSCQP_DAS_KERNARGS();  // (one block of kernel-argument reads, one wait: lscqp_das.hpp)
    const int64_t k0 = blockIdx.x;
    if (k0 >= n) return;
    const int64_t q = ka_order ? (int64_t)ka_order[k0] : k0;
#else
    const int64_t k0 = blockIdx.x;
    if (k0 >= n) return;
    const int64_t q = cls.order ? (int64_t)cls.order[k0] : k0;
#endif
    int verdict = kDasSolved;
    {  // the phase: das_kernel<4, false, false, false>'s body (lscqp_das_body.inc) with the class's shape as constants and nothing in front
        using FC = FusedCarve<M, DIM, ES, NSLOT, W>;
        constexpr int NW = 4, T = 64 * NW;
        // Row slots per thread, from the carve: as many as a full instance's rows need, at most four.  The 600-row forms get three -- a
        // fourth would load, translate, stage-test and evaluate a row that cannot exist, in the prologue and in every pass; the 2 400-row
        // form keeps four and loops.  (The pass's (slack, id) minimum is lexicographic: it does not depend on which thread saw which row.)
        constexpr int kU = (FC::kStage + T - 1) / T < 4 ? (FC::kStage + T - 1) / T : 4;
        constexpr bool F32 = false, SCREEN = false, PEEL = false;
        constexpr int dim = DIM, es = ES ? 1 : 0, behind = 0;
        constexpr int kMaxNL = FC::kStage;  // (an instance beyond the launch's cap <= MAX_OBS is handed over before its rows are read)
        // fewer than four slots: one block of kU * T rows holds every row of an instance the phase accepts (the first pass has no further trip)
        static_assert(kU == 4 || kMaxNL <= kU * T, "the row slots must cover the carve's staged rows");
        static_assert(kU >= 1, "an instance has rows");
#define LSCQP_DAS_END(verdict_)   \
    do {                          \
        verdict = (verdict_);     \
        goto phase_done;          \
    } while (0)
#define LSCQP_DAS_LAYOUT Layout::make(M, DIM, FC::KMAX, 1, FC::kStage)
#include "lscqp_das_body.inc"
#undef LSCQP_DAS_LAYOUT
#undef LSCQP_DAS_END
    }
phase_done:
    // (the verdict is the same in every thread: each exit of the phase is taken by the whole workgroup)
    verdict = __builtin_amdgcn_readfirstlane(verdict);
    if (verdict != kDasHandedOver) return;
    // Every wavefront is done with the phase's LDS before the interior-point instance lays out its own over it, and the status thread 0
    // stored (ITER_LIMIT) is visible to the lanes of lscqp_pdip_one, which read it again: __syncthreads() is a workgroup-scope release, the
    // barrier, a workgroup-scope acquire.
    __syncthreads();
    // The wavefronts beyond W leave.  The barriers of lscqp_pdip_one then wait for the W that remain: S_BARRIER waits only for the waves of
    // the workgroup that have not ended (CDNA4 ISA, S_BARRIER).  (readfirstlane: a wave-uniform exit, one s_endpgm per leaving wavefront.)
    if constexpr (W < 4) {
        if (__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) >= W) return;
    }
    lscqp::lscqp_pdip_one<M, DIM, ES, NSLOT, W, double>(cls, q, smem, hdr, rows, row_offsets, sfc, x_init, x_out, obj_out, status_out, info_out);
}

}  // namespace lscqp_das

// cls: the class of the interior-point pass (repair = 3, no queue, no scan; the phase reads none of those fields).  The phase's launch
// parameters are those of lscqp_launch_das with threads = 256, the first look inside the loop of steps, fp64 rows, nothing in front.
// Returns hipErrorNotSupported -- and launches nothing -- when the budgets exceed the phase's compiled carve (FusedCarve: kmax, stage_rows),
// the two LDS footprints do not fit one CU or the instance cannot hold the batch; the caller then launches the two kernels.
extern "C" hipError_t LSCQP_FUSED_FN(const lscqp::DevClass* cls, int cap, int kmax, int max_steps, int cacheC, int stage_rows, const double* d_tab,
                                     int64_t n, const lscqp_header* hdr, const lscqp_row* rows, const uint64_t* row_offsets, const lscqp_box* sfc,
                                     const double* x_init, double* x_out, double* obj_out, int32_t* status_out, lscqp_info* info_out,
                                     hipStream_t stream) {
    using C = lscqp::Cfg<LSCQP_M, LSCQP_DIM, (LSCQP_ES != 0), LSCQP_NSLOT, LSCQP_W, (int)sizeof(double)>;
    using FC = lscqp_das::FusedCarve<LSCQP_M, LSCQP_DIM, (LSCQP_ES != 0), LSCQP_NSLOT, LSCQP_W>;
    auto kern = lscqp_das::das_pdip_kernel<LSCQP_M, LSCQP_DIM, (LSCQP_ES != 0), LSCQP_NSLOT, LSCQP_W>;
    if (kmax < 1 || kmax > lscqp_das::kMaxK || cls->rows_f32 || cls->queue || cls->scan || cls->repair != 3) return hipErrorInvalidValue;
    if (cls->n_obs_max > C::MAX_OBS || cap > C::MAX_OBS) return hipErrorNotSupported;
    if (kmax > FC::KMAX || stage_rows > FC::kStage) return hipErrorNotSupported;  // (beyond the compiled carve)
    const size_t lds_das = sizeof(double) * (size_t)lscqp_das::Layout::make(LSCQP_M, LSCQP_DIM, FC::KMAX, 1, FC::kStage).total;
    const size_t lds = lds_das > C::lds_bytes() ? lds_das : C::lds_bytes();
    if (lds > lscqp::kMaxLdsBytes) return hipErrorNotSupported;
    static std::atomic<bool> attr_set[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    if (!attr_set[dev].load(std::memory_order_acquire)) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lscqp::kMaxLdsBytes);
        if (e != hipSuccess) return e;
        attr_set[dev].store(true, std::memory_order_release);
    }
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(kern, dim3((unsigned)n), dim3(256), lds, stream, *cls, cap, kmax, max_steps, cacheC, stage_rows, d_tab, n, hdr, rows, row_offsets, sfc,
                       x_init, x_out, obj_out, status_out, info_out);
    return hipGetLastError();
}

#ifdef LSCQP_DAS_TIMING
// the phase's cycle totals of this fused instance (one instance per library: tools/das_timing.py builds the twin of one)
extern "C" int lscqp_das_fused_cycles(unsigned long long* out, int reset) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(lscqp_das::das_fused_cycles), sizeof(unsigned long long) * 16);
    if (reset) {
        unsigned long long z[16] = {0};
        (void)hipMemcpyToSymbol(HIP_SYMBOL(lscqp_das::das_fused_cycles), z, sizeof z);
    }
    return 0;
}
#endif
