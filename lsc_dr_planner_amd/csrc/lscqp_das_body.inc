// lscqp_das_body.inc — the dual active-set phase on ONE instance q, by the workgroup of 64 * NW threads (lscqp_das.hpp).
// Included textually into the body of a kernel -- das_kernel, and lscqp_fused.hip's das_pdip_kernel -- where these are in scope:
//   NW, F32, SCREEN, PEEL, T = 64 * NW, kU, kMaxNL (constants; kMaxNL bounds an instance's LSC rows); cls, M, dim, es, cap, kmax, max_steps,
//   cacheC, stage_rows, behind, tab, q, hdr, rows, row_offsets, sfc, x_init, x_out, obj_out, status_out, info_out; smem (the dynamic LDS,
//   lscqp_das_lds_bytes(M, dim, kmax, cacheC, stage_rows), or the carve of LSCQP_DAS_LAYOUT);
//   LSCQP_DAS_FORM: which of the phase's TWO texts the kernel compiles (the values' names are lscqp_das.hpp's).
//   LSCQP_DAS_THROUGHPUT -- das_kernel in every form and the fused form <10,3,1,10,4>: every value is read where it is used, and nothing
//   is set up for a first step ahead of it.  das_kernel's forms serve the batches that fill the chip, where a quiet instance must not
//   pay for step setup, and every one-wavefront form came out worse with the kernel-argument block (NOTES section 23).
//   LSCQP_DAS_LATENCY -- the fused forms <5,3,1,5,2> and <10,2,1,5,2>, batches of at most one instance per CU, where ONE instance that
//   takes steps is the launch's time.  What this text does differently:
//     - the prologue (everything above DAS_T(1)) is scheduled around the kernel-argument block of LSCQP_DAS_KERNARGS (lscqp_das.hpp:
//       ka_dt, ka_q2s, ka_w_t, ka_w_c, ka_comm_range, ka_use_sfc, ka_rsfc, ka_wb0 .. 5, ka_roffs, ka_sfc), which the kernel has placed in
//       front of its exit test: one wave of clamped, untested loads, and the phase reads no field of cls and neither row_offsets nor sfc
//       by name (NOTES section 23, profiles/r15_prologue.txt);
//     - what the first step needs and only the header decides is done ahead of it: the factor zeroed in the prologue, the class's
//       table left in LDS by the first pass where it fits the registers; a joining row's descriptors are stored from registers, not
//       copied from the candidate's slot (section 24, profiles/r16_step_path.txt);
//     - the verification is straight-line code -- every operand asked for before the first arithmetic, lam_ kept zero from the
//       prologue on instead of zeroed behind a barrier of its own -- and the objective's rounding term comes from one block of loads
//       instead of a loop of six dependent ones (section 31, profiles/r23_verification.txt);
//     - LDS round trips that held one or two reads are folded: the four empty-interval ballots in one read without a branch; the
//       pass's minimum across the wavefronts from one block of reads, by selects; `primal` read with t, kind and l in front of the test
//       on kind; a two-sided candidate's stencil and both bounds asked for together; the candidate's multiplier so far in a register
//       of wavefront 0 beside ctl_[3] (section 35, profiles/r27_round_trips.txt);
//     - the thread's two-sided rows sit in registers from the prologue on, and its LSC rows -- translated once in front of the loop of
//       steps -- with their positions in c_: a later pass reads no staged row (the stores to the staged arrays stay: decode reads the
//       candidate's row there), and the first pass, as the later one, asks for every operand in c_ in one block of requests (sections
//       35 and 40, profiles/r31_row_registers.txt).
//   The two texts differ in WHEN, and by which thread, a value is asked for, moved and waited for: no expression that rounds, no order
//   of a sum or a comparison, no barrier's place.  Every form of the phase therefore returns the same bytes (tests/test_das_prologue.py,
//   test_das_step_path.py, test_das_verification.py, test_das_round_trips.py, test_das_row_registers.py).  Each change was once a setting
//   of its own, so that a timing twin could be built with it alone: NOTES section 42 says what became of those settings.
//   The latency text needs the compile-time carve (LSCQP_DAS_LAYOUT), four wavefronts, and a shape whose LSC rows and two-sided rows fit
//   one block of row slots each: checked once, below.
//   LSCQP_DAS_END(verdict): leaves the phase with a DasVerdict, taken by the whole workgroup at once;
//   LSCQP_DAS_LAYOUT (optional): the LDS carve as a constant expression, with room for at least kmax active rows, the class's table and
//   stage_rows staged rows; without it the carve is made at run time from kmax, cacheC and stage_rows.  kmax, max_steps, cacheC and
//   stage_rows are the launch's BUDGETS either way: the carve's capacities (L.kmax, L.n_stage) only place the arrays.
// (Text, not a function: the kernel's own code then is exactly what it was as one function -- a __forceinline__ device function holding this
// body was simplified before it was inlined, through a generic LDS pointer, and das_kernel came out 2 VGPRs and some SGPR spills different
// and the 512-QP batches 2 % slower, measured.)
#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
#define DAS_CLS(f) ka_##f  // a scalar of the class: the kernel-argument block's register
// the wavefront's reductions on DPP steps without identity moves (lscqp_das.hpp): the same trees, the same bits
#define DAS_ARGMIN wave_argmin_ror
#define DAS_SUM(v) wave_reduce1_zero<lscqp::OpSum>(v)
#define DAS_MAX0(v) wave_reduce1_zero<OpMax0>(v)  // (a maximum over values >= +0.0)
#define DAS_MAX0_MAX0_SUM(a, b, c) wave_reduce3_zero<OpMax0, OpMax0, lscqp::OpSum>(a, b, c)
#elif LSCQP_DAS_FORM == LSCQP_DAS_THROUGHPUT
#define DAS_CLS(f) cls.f  // a scalar of the class: the kernel argument, read where it is used
#define DAS_ARGMIN wave_argmin
#define DAS_SUM(v) wave_sum(v)
#define DAS_MAX0(v) wave_max(v)
#define DAS_MAX0_MAX0_SUM(a, b, c) lscqp::wave_reduce3<lscqp::OpMax, lscqp::OpMax, lscqp::OpSum>(a, b, c)
#else
#error "LSCQP_DAS_FORM is LSCQP_DAS_THROUGHPUT or LSCQP_DAS_LATENCY"
#endif
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#ifdef LSCQP_DAS_LAYOUT
    constexpr Layout L = LSCQP_DAS_LAYOUT;
#else
    const Layout L = Layout::make(M, dim, kmax, cacheC, stage_rows);
#endif
    constexpr int kPB = 4;  // two-sided rows a thread asks for in one block (the prologue's, and each trip of the section that computes them)
#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
    // ---- what the latency text needs, all of it ----
#ifndef LSCQP_DAS_LAYOUT
#error "the latency text sizes its register copies of the rows, and places the class's table, from the compile-time carve"
#endif
    // four wavefronts: the folded reads take four ballots, four minima and four ids; the first pass's barrier publishes the table; the
    // objective's lanes are the second wavefront's; the stationarity rows take one trip of the workgroup
    static_assert(NW == 4, "the latency text is the four-wavefront form's");
    static_assert(kMaxNL <= kU * T, "one block of row slots holds every LSC row of the shape: the thread's rows stay in registers");
    static_assert(L.NPAIR <= kPB * T, "the prologue's one block of slots holds every two-sided row of the shape");
    static_assert(L.o_red % 2 == 0, "the folded reads of red_ are 16-byte words");
    // (the class's table: where it fits the registers, cpre[] is loaded whatever cacheC says -- the latency prologue's c_fits -- and the
    // first pass stores it from there: kTableEarly, below, needs nothing else)
#endif
    DAS_T_DECL();
    const int P = L.P, NX = L.NX, NPAIR = L.NPAIR;
    const int kcap = L.kmax;  // active rows the carve holds (>= the budget kmax); slot kcap of the descriptors is the candidate's
    double* const H_ = smem + L.o_hdr;
    double* const sfc_ = smem + L.o_sfc;
    double* const c_ = smem + L.o_c;
    double* const cu_ = smem + L.o_cu;
    double* const lam_ = smem + L.o_lam;
    double* const plo_ = smem + L.o_plo;
    double* const phi_ = smem + L.o_phi;
    int* const pix_ = reinterpret_cast<int*>(smem + L.o_pix);  // packed stencil of a two-sided row: type << 24 | first entry index (in 0 .. NX-1) << 12 | second
    double* const W_ = smem + L.o_W;   // [kcap + 1][NX]
    double* const Jm_ = smem + L.o_L;  // [kcap][kcap + 1] J = L^-1, S = A'C A = L L' over the active rows
    double* const u_ = smem + L.o_u;
    double* const r_ = smem + L.o_r;
    double* const arhs_ = smem + L.o_arhs;    // [kcap + 1]: slot kcap = the candidate row
    double* const acoef_ = smem + L.o_acoef;  // [kcap + 1][3]
    int* const aint_ = reinterpret_cast<int*>(smem + L.o_aint);  // [kcap + 1][4]: id, entry0, entry1, entry2
    double* const red_ = smem + L.o_red;      // [2][16]
    double* const ctl_ = smem + L.o_ctl;      // step decision of wavefront 0: t, kind, leaving row, accumulated multiplier of the candidate
    double* const wb_ = smem + L.o_wb;
    double* const dq_ = smem + L.o_dq;        // world_min[3], world_max[3]
    double* const Cc_ = smem + L.o_C;
    double* const Sx_ = smem + L.o_rows;      // staged LSC rows: [nx | ny | nz | b] x stage_rows
    double* const Sy_ = Sx_ + L.n_stage;
    double* const Sz_ = Sy_ + L.n_stage;
    double* const Sb_ = Sz_ + L.n_stage;
    const int LDL = kcap + 1;
    int par = 0;  // which half of red_ the next cross-wavefront reduction uses (double buffered: one barrier per reduction)

    if (!SCREEN && behind) {  // (uniform) behind the lean form (bit 0): what it finished is skipped before anything is fetched; behind the
        const int st_early = status_out[q];  // prescreen (bit 1, lscqp_prescreen.hip): so is what it proved infeasible
        if ((behind & 1) && st_early == LSCQP_STATUS_OPTIMAL) LSCQP_DAS_END(kDasSolved);
        if ((behind & 2) && st_early == LSCQP_STATUS_INFEASIBLE) LSCQP_DAS_END(kDasInfeasible);
    }
#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
    // ---- ONE wave of requests: the instance's row offset and obstacle count, the class's two-sided rows, the header, the corridor
    // boxes and the objective's rounding terms -- straight-line code, every address clamped into memory the instance owns, no test around
    // any load (a branch around a load makes the compiler wait for every load right behind it: the loads have to be in flight TOGETHER).
    // Vector loads return in the order they were asked for, so the LSC rows are asked for LAST, as soon as offset and count are there: the
    // wait for the header then leaves them in flight, across the barrier and under everything up to the first pass.
    // (offset and count are per-thread vector loads of one address, not scalar loads: they stand FIRST in the machine code, and the wait
    // in front of the rows' addresses is for these two alone -- the other four stay in flight.  n_obs, in_cap, nL and roff therefore live in
    // vector registers and are divergent to the compiler, uniform in fact: NOTES section 23.)
    const lscqp_header* const hq = hdr + q;
    const bool use_sfc = ka_use_sfc != 0;  // (uniform)
    constexpr int kNS = (72 + T - 1) / T;  // corridor-box words per thread (6 M <= 72)
    LSCQP_DAS_GLOBAL const double* const hsrc = (LSCQP_DAS_GLOBAL const double*)hq;
    LSCQP_DAS_GLOBAL const double* const ssrc = use_sfc ? ka_sfc + q * 6 * M : hsrc;  // (no boxes: the header again, unused)
    double hw = hsrc[tid & 31];
    double sw[kNS];
#pragma unroll
    for (int i = 0; i < kNS; i++) sw[i] = ssrc[(use_sfc && tid + i * T < 6 * M) ? tid + i * T : 0];
    const double* const tab_end = tab + (size_t)M * table_stride(M);  // (behind the tables: lscqp_api.hip, das_refresh)
    double dqw = tab_end[min(tid, 35)];
    // the class's two-sided rows (lscqp_das_build_pairs, behind the tables and the 36 rounding terms): the first four of this thread
    const int2* const pairs_g = reinterpret_cast<const int2*>(tab_end + 36);
    int2 pwr[kPB];
#pragma unroll
    for (int u = 0; u < kPB; u++) pwr[u] = pairs_g[min(tid + u * T, NPAIR - 1)];
    // (offset and count: the compiler moves these two to the head of the wave)
    const uint64_t roff_raw = *(ka_roffs ? ka_roffs + q : (LSCQP_DAS_GLOBAL const uint64_t*)hq);  // (no offsets: a word of the header, unused)
    const int n_obs = hq->n_obs;
    // the first LSC rows of this thread, raw.  An instance beyond the launch's capacity is handed over below and NO row of it is asked for;
    // neither is one where the instance has none: those loads read the head of the instance's own header and their values are dropped.
    __builtin_amdgcn_sched_barrier(0);  // (everything above is asked for before the first wait below)
    const uint64_t roff = ka_roffs ? roff_raw : 0;
    const bool in_cap = !(n_obs > cap || n_obs < 0);
    const int nL = in_cap ? n_obs * P : 0;
    auto fetch_row = [&](int j, double& x, double& y, double& z, double& w) {  // raw row j of this instance
        if constexpr (F32) {
            const float4 f = reinterpret_cast<const float4*>(rows)[roff + (uint64_t)j];
            x = f.x, y = f.y, z = f.z, w = f.w;
        } else {
            const double4 d = *reinterpret_cast<const double4*>(&rows[roff + (uint64_t)j]);
            x = d.x, y = d.y, z = d.z, w = d.w;
        }
    };
    double px[kU], py[kU], pz[kU], pw[kU];
    {
        using RowT = std::conditional_t<F32, float4, double4>;
        const RowT* const rbase = nL > 0 ? reinterpret_cast<const RowT*>(rows) + roff : reinterpret_cast<const RowT*>(hq);
#pragma unroll
        for (int u = 0; u < kU; u++) {
            const int j = tid + u * T;
            const RowT d = rbase[j < nL ? j : 0];
            px[u] = nL > 0 ? (double)d.x : 0.0, py[u] = nL > 0 ? (double)d.y : 0.0, pz[u] = nL > 0 ? (double)d.z : 0.0, pw[u] = nL > 0 ? (double)d.w : -1.0;
        }
    }
    // ONE wait for the wave, with the rows left in flight (the values are taken here: left alone, the compiler moves a load into the test
    // around its store, with a wait for everything behind it)
    asm volatile("" : "+v"(hw), "+v"(dqw));
#pragma unroll
    for (int i = 0; i < kNS; i++) asm volatile("" : "+v"(sw[i]));
    if (tid < 32) H_[tid] = hw;
#pragma unroll
    for (int i = 0; i < kNS; i++)
        if (use_sfc && tid + i * T < 6 * M) sfc_[tid + i * T] = sw[i];
    if (tid < 36) dq_[tid] = dqw;
    if (tid == 0) {  // (registers of the kernel-argument block)
        wb_[0] = ka_wb0, wb_[1] = ka_wb1, wb_[2] = ka_wb2, wb_[3] = ka_wb3, wb_[4] = ka_wb4, wb_[5] = ka_wb5;
        // four class scalars for the verification, which reads them from here instead of holding eight scalar registers across the loop of
        // steps (or reading them again from the kernel-argument segment, with a wait the LDS reads around it share): slots nothing else uses
        wb_[6] = ka_dt, wb_[7] = ka_q2s, ctl_[4] = ka_w_t, red_[44] = ka_w_c;
    }
    LSCQP_DAS_BARRIER();
#else
    // ---- header, corridor boxes (and the instance's row offset: one memory round trip for all three) -------------------------------
    const uint64_t roff = row_offsets ? row_offsets[q] : 0;
    // the class's two-sided rows (lscqp_das_build_pairs, behind the tables and the 36 rounding terms): the first four of this thread are asked
    // for NOW -- they depend on nothing the header holds
    const int2* const pairs_g = reinterpret_cast<const int2*>(tab + (size_t)M * table_stride(M) + 36);
    int2 pwr[kPB];
#pragma unroll
    for (int u = 0; u < kPB; u++) pwr[u] = pairs_g[min(tid + u * T, NPAIR - 1)];
    {
        const double* hsrc = reinterpret_cast<const double*>(hdr + q);
        const double* ssrc = reinterpret_cast<const double*>(sfc) + q * 6 * M;
        for (int e = tid; e < 32 + (cls.use_sfc ? 6 * M : 0); e += T) (e < 32 ? H_[e] : sfc_[e - 32]) = e < 32 ? hsrc[e] : ssrc[e - 32];
        if (tid >= 64 - 36 && tid < 64) dq_[tid - (64 - 36)] = tab[(size_t)M * table_stride(M) + (tid - (64 - 36))];  // (behind the tables: lscqp_api.hip, das_refresh)
        if (tid < 6) {  // (selects, not an indexed kernel argument)
            const double w = tid == 0 ? cls.world_min[0] : tid == 1 ? cls.world_min[1] : tid == 2 ? cls.world_min[2] : tid == 3 ? cls.world_max[0] : tid == 4 ? cls.world_max[1] : cls.world_max[2];
            wb_[tid] = w;
        }
    }
    __syncthreads();
#endif
    DAS_T(0);  // header, boxes, row offset
    const lscqp_header* Hd = reinterpret_cast<const lscqp_header*>(H_);
    const lscqp_box* sfcl = reinterpret_cast<const lscqp_box*>(sfc_);
#if LSCQP_DAS_FORM == LSCQP_DAS_THROUGHPUT
    const int n_obs = Hd->n_obs;
#endif
    // Handing an instance over: the interior-point kernel behind this phase solves whatever is not OPTIMAL (cls.repair == 3 there).
    // (why: LSCQP_DAS_WHY_* of include/lscqp.h, left in lscqp_info.res_dual of an instance nobody solves afterwards -- LSCQP_ACTIVE_SET_ONLY,
    // tests and tools/loaded_probe.py; the pass that solves the instance overwrites the record)
    auto hand_over = [&](int steps, int why) {
        for (int e = tid; e < NX; e += T) x_out[q * NX + e] = x_init ? x_init[q * NX + e] : Hd->p0[fdiv(e, 1.0f / (float)P)];
        if (tid == 0) {
            obj_out[q] = 0.0;
            status_out[q] = LSCQP_STATUS_ITER_LIMIT;
            if (info_out) {
                info_out[q].iterations = 0;
                info_out[q].flags = 0;
                info_out[q].res_primal = 0.0;
                info_out[q].res_dual = (double)why;
                info_out[q].gap = (double)steps;  // (overwritten by the pass that solves the instance)
            }
        }
    };
    // An instance whose row system has no point, PROVEN inside the phase (an empty interval; a violated row whose normal lies in the span of
    // the active rows' with no multiplier to give way: a Farkas certificate, taken only where the violation exceeds 1e-6 m plus what the
    // normal's part outside that span could buy across the world box -- see kind 3): LSCQP_STATUS_INFEASIBLE here and now, nothing left
    // for the kernel behind.  The
    // reference's caller keeps initial_traj for any failure (src/traj_planner.cpp:767-797); x_out is the handed-over start, as above.
    auto infeasible_out = [&](int steps, double violation) {
        for (int e = tid; e < NX; e += T) x_out[q * NX + e] = x_init ? x_init[q * NX + e] : Hd->p0[fdiv(e, 1.0f / (float)P)];
        if (tid == 0) {
            obj_out[q] = 0.0;
            status_out[q] = LSCQP_STATUS_INFEASIBLE;
            if (info_out) {
                info_out[q].iterations = steps;
                info_out[q].flags = LSCQP_INFO_ACTIVE_SET;
                info_out[q].res_primal = violation;
                info_out[q].res_dual = 0.0;
                info_out[q].gap = 0.0;
            }
        }
    };
#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
    if (!in_cap)
#else
    if (n_obs > cap || n_obs < 0)
#endif
    {  // the kernel instance behind this phase refuses it (LSCQP_STATUS_CAPACITY): its verdict, not ours
        hand_over(0, LSCQP_DAS_WHY_CAPACITY);
        LSCQP_DAS_END(kDasHandedOver);
    }
    const double dt = DAS_CLS(dt);
    const double org0 = Hd->p0[0], org1 = Hd->p0[1], org2 = Hd->p0[2];
    const double* const org = Hd->p0;  // (LDS: indexed with a run-time axis; a register array would be materialised in scratch memory)
    int ts = Hd->terminal_segments;
    if (ts <= 0) {  // src/traj_optimizer.cpp:530-538 in fp64 (as lscqp_kernel.hpp)
        const double g0 = Hd->goal[0] - org0, g1 = Hd->goal[1] - org1, g2 = Hd->goal[2] - org2;
        ts = (int)((M * dt - sqrt(g0 * g0 + g1 * g1 + g2 * g2) / Hd->nominal_velocity + 1e-9) / dt);
        if (ts < 1) ts = 1;
    }
    if (ts > M) ts = M;
    const double q2s = DAS_CLS(q2s), wt2 = 2.0 * DAS_CLS(w_t);
    const double* const tb = tab + (size_t)(ts - 1) * table_stride(M);
    const double* const U1 = tb, * const U2 = tb + P, * const G1 = tb + 2 * P, * const Cg = tb + 3 * P;
    const bool comm_on = DAS_CLS(comm_range) > 0;
    const double rho_pair = 0.5 * DAS_CLS(comm_range) - Hd->radius;  // :484
    const double rho_wp = 0.5 * DAS_CLS(comm_range) - 1e-5;          // :495
#if LSCQP_DAS_FORM == LSCQP_DAS_THROUGHPUT
    const int nL = n_obs * P;
#endif
    const float iP = 1.0f / (float)P;
    const bool staged = stage_rows > 0 && nL <= stage_rows;  // (uniform)
    bool rows_in_lds = false;                                // set by the first pass

#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
    // ---- behind the rows, and under their trip: the table vectors of this thread's control points (they need ts), clamped, no test ----
    constexpr int NE = 4;  // control-point entries per thread the prologue handles in registers (NX <= 4 T for every shape: 216 at M = 12 in 3-D)
    double tu1[NE], tu2[NE], tg1[NE];
#pragma unroll
    for (int i = 0; i < NE; i++) {
        const int e = tid + i * T < NX ? tid + i * T : 0;
        const int cp = e - P * fdiv(e, iP);
        tu1[i] = U1[cp], tu2[i] = U2[cp], tg1[i] = G1[cp];
    }
#else
    // ---- memory first: the table vectors of this thread's control points and its first LSC rows are requested before anything is computed --
    // (the row format is a template parameter and the index is clamped instead of guarded: a branch around a load makes the compiler wait
    // for every load right behind it -- the loads of a thread have to be in flight TOGETHER)
    auto fetch_row = [&](int j, double& x, double& y, double& z, double& w) {  // raw row j of this instance
        if constexpr (F32) {
            const float4 f = reinterpret_cast<const float4*>(rows)[roff + (uint64_t)j];
            x = f.x, y = f.y, z = f.z, w = f.w;
        } else {
            const double4 d = *reinterpret_cast<const double4*>(&rows[roff + (uint64_t)j]);
            x = d.x, y = d.y, z = d.z, w = d.w;
        }
    };
    constexpr int NE = 4;  // control-point entries per thread the prologue handles in registers (NX <= 4 T for every shape: 216 at M = 12 in 3-D)
    double tu1[NE], tu2[NE], tg1[NE];
#pragma unroll
    for (int i = 0; i < NE; i++) {
        const int e = tid + i * T;
        if (e < NX) {
            const int cp = e - P * fdiv(e, iP);
            tu1[i] = U1[cp], tu2[i] = U2[cp], tg1[i] = G1[cp];
        }
    }
    double px[kU], py[kU], pz[kU], pw[kU];  // the first rows of this thread, raw
#pragma unroll
    for (int u = 0; u < kU; u++) px[u] = py[u] = pz[u] = 0.0, pw[u] = -1.0;
    if (nL > 0) {
#pragma unroll
        for (int u = 0; u < kU; u++) {
            const int j = tid + u * T;
            fetch_row(j < nL ? j : 0, px[u], py[u], pz[u], pw[u]);
        }
    }
#endif

    // The small-batch form asks for the class's table NOW as well (an instance with a step would otherwise wait a memory round trip for it at
    // its first step -- and in a batch of 64 that one instance is the launch's time); a quiet instance never waits for these loads.
    constexpr int kCPre = (NW == 4 && !PEEL && !SCREEN) ? 6 : 0;  // table entries per thread held in registers (6 x 256 >= 36 M^2 up to M = 6)
    double cpre[kCPre > 0 ? kCPre : 1];
#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
    const bool c_fits = kCPre > 0 && P * P <= kCPre * T;  // (uniform; a constant of the shape: the loads then stand in straight-line code)
    const bool c_prefetched = c_fits && cacheC;           // (uniform; the fused forms always keep the table)
    // What the first step needs and only the header decides, done under the rows' trip instead of on the stepping instance's path: the
    // factor zeroed by every thread (below, behind c_u; it was wavefront 0's, 17 stores per lane, in front of the first candidate), and --
    // where the table fits the registers asked for here -- the table left in LDS by the first pass (in front of that pass's barrier,
    // which publishes it) whatever cacheC says: the compile-time carve has the room, and the values are the table's own either way.
    // A quiet instance now waits for the table's loads; in a batch of at most one instance per CU its time is not the launch's.
    // (this text asks for the table whatever cacheC says: the other one would leave cpre[] unset at cacheC == 0)
    constexpr bool kTableEarly = kCPre > 0 && L.P * L.P <= kCPre * T;
#else
    const bool c_prefetched = kCPre > 0 && cacheC && P * P <= kCPre * T;  // (uniform)
    const bool c_fits = c_prefetched;
    constexpr bool kTableEarly = false;
#endif
    if constexpr (kCPre > 0) {
        if (c_fits) {
#pragma unroll
            for (int i = 0; i < kCPre; i++) {
                const int e = tid + i * T;
                cpre[i] = Cg[e < P * P ? e : 0];
            }
        }
    }

    // ---- the two-sided rows, one table for all four families (ids nL + 2 r + side; side 0: stencil - lo >= 0, side 1: hi - stencil >= 0) ----
    //   r in [0, NX)                    interval of one control point: world box, corridor, communication rows on c[m][5]  (:252-265, 372-397, 482-497)
    //   then dim * 5M velocity rows     c[i+1] - c[i],            |.| <= vmax dt / n          (:448-453)
    //   then dim * 4M acceleration rows c[i+2] - 2 c[i+1] + c[i], |.| <= amax dt^2 / (n (n-1)) (:462-471)
    //   then dim * NCP pairs (uu, up)   c[uu][5] - c[up+1][0],    |.| <= rho                   (:482-487 with mi = up + 1 >= 1)
    // type 0: no row; 1: interval; 2: velocity; 3: acceleration; 4: pair.  Entry indices are positions in c_ (axis * P + control point).
    bool empty = false;
    const double hv_c = dt * 0.2, ha_c = dt * dt * 0.05;
#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
    // This thread's two-sided rows stay in registers across the loop of steps -- they never change after this section, which computes and
    // stores them anyway: the packed stencil, its three positions in c_ and two coefficients (pair_val's), lo, hi.  A slot without a row
    // (r >= NPAIR) holds stencil 0: no row.  Sized from the shape, as kU is: one slot at M = 5 in 3-D (255 rows), two at M = 10 in 2-D (320);
    // the section's first block of kPB slots holds every row of the shape.
    constexpr int kPR = (L.NPAIR + T - 1) / T;
    int tp_pk[kPR], tp_i0[kPR], tp_i1[kPR], tp_e0[kPR];
    double tp_a1[kPR], tp_a2[kPR], tp_lo[kPR], tp_hi[kPR];
#pragma unroll
    for (int u = 0; u < kPR; u++)  // (a thread behind the last row never enters the section's loop)
        tp_pk[u] = tp_i0[u] = tp_i1[u] = tp_e0[u] = 0, tp_a1[u] = tp_a2[u] = tp_lo[u] = tp_hi[u] = 0.0;
#endif
    for (int r0 = tid; r0 < NPAIR; r0 += kPB * T) {
        if (r0 != tid) {
#pragma unroll
            for (int u = 0; u < kPB; u++) pwr[u] = pairs_g[min(r0 + u * T, NPAIR - 1)];
        }
#pragma unroll
        for (int u = 0; u < kPB; u++) {
            if ((r0 - tid) + u * T >= NPAIR) break;  // (uniform: no thread of the workgroup has a row in this slot)
            const int r = r0 + u * T;
            const int w0 = pwr[u].x, w1 = pwr[u].y;
            const int fam = w1 & 3, k = (w1 >> 2) & 3, m = (w1 >> 4) & 15;
            const bool last = (w1 >> 8) & 1, rs = (w1 >> 9) & 1;
            // every load of every family, without a test (one branch per family made the compiler wait for each family's loads in turn)
            const double ok_ = org[k], wlo = wb_[k], whi = wb_[3 + k], wpk = Hd->next_waypoint[k] - ok_;
            const double hv = Hd->vmax[k] * hv_c, ha = Hd->amax[k] * ha_c;
            double lo = wlo - ok_, hi = whi - ok_;  // :252-253,260-265
            if (DAS_CLS(rsfc) && rs) {          // :255-258
                lo = -100.0 - ok_;
                hi = 100.0 - ok_;
            }
            if (DAS_CLS(use_sfc)) {  // (uniform) :372-397
                lo = fmax(lo, sfcl[m].bmin[k] - ok_);
                hi = fmin(hi, sfcl[m].bmax[k] - ok_);
            }
            const double clo = fmax(lo, fmax(-rho_pair, wpk - rho_wp)), chi = fmin(hi, fmin(rho_pair, wpk + rho_wp));  // pairs (m, mi = 0) :482-487, waypoint rows :494-497
            lo = (comm_on && last) ? clo : lo;
            hi = (comm_on && last) ? chi : hi;
            const double hs = fam == 1 ? hv : fam == 2 ? ha : rho_pair;  // :448-453, :462-471, :482-487
            lo = fam == 0 ? lo : -hs;
            hi = fam == 0 ? hi : hs;
            if (r < NPAIR) {
                if (fam == 0 && (w0 >> 24) != 0 && lo > hi) empty = true;
                plo_[r] = lo, phi_[r] = hi;
                pix_[r] = w0;
            }
#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
            if (u < kPR) {  // (a constant of the unrolled loop; r = tid + u T here: the section has one block)
                const int pk = r < NPAIR ? w0 : 0;
                const int type = pk >> 24, e0 = (pk >> 12) & 0xfff, e1 = pk & 0xfff;  // (pair_val's decoding, below)
                const int us = u < kPR ? u : 0;  // (the index stays inside the arrays in the unrolled copies this test removes)
                tp_pk[us] = pk;
                tp_i0[us] = (type == 4) ? e1 : e0 + max(type - 1, 0);
                tp_i1[us] = (type == 3) ? e0 + 1 : e0;
                tp_e0[us] = e0;
                tp_a1[us] = (type <= 1) ? 0.0 : (type == 3) ? -2.0 : -1.0;
                tp_a2[us] = (type == 3) ? 1.0 : 0.0;
                tp_lo[us] = lo, tp_hi[us] = hi;
            }
#endif
        }
    }
    // ---- unconstrained optimum: c_u[k] = cfix[k] - c1_k U1 - c2_k U2 + 2 w_t goal_k G1 ---------------------------------------------------
#pragma unroll
    for (int i = 0; i < NE; i++) {
        const int e = tid + i * T;
        if (e < NX) {
            const int k = fdiv(e, iP), cp = e - k * P;
            const double c1 = Hd->v0[k] * dt * 0.2;
            const double c2 = Hd->a0[k] * dt * dt * 0.05 + 2.0 * c1;
            const double fixv = (cp == 1) ? c1 : (cp == 2) ? c2 : 0.0;
            const double cv = fixv - c1 * tu1[i] - c2 * tu2[i] + wt2 * (Hd->goal[k] - org[k]) * tg1[i];
            c_[e] = cv;
            cu_[e] = cv;
        }
    }
    if (dim == 2)
        for (int e = tid; e < P; e += T) c_[2 * P + e] = 0.0;
#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
    {  // the factor, zeroed behind the section's own LDS traffic, two entries a store (k (k + 1) is even, the carve aligns to 16 bytes)
        double2* const J2 = reinterpret_cast<double2*>(Jm_);
        for (int e = tid; e < kcap * LDL / 2; e += T) J2[e] = make_double2(0.0, 0.0);
    }
    // A'u is zero wherever no multiplier is held: the verification reads lam_ without a test and thread 0 adds to it without zeroing it
    // first (finish_local).  The barrier below publishes the zeros; whoever verifies a second time restores them (the polish path).
    for (int e = tid; e < NX; e += T) lam_[e] = 0.0;
    // the workgroup's verdict on `empty` with ONE barrier: every wavefront leaves its own ballot in a slot of red_ no reduction uses
    // ([20, 24) of the first half), every thread reads all of them behind the barrier that also publishes c_ and the two-sided rows
    const bool empty_w = __ballot(empty) != 0;  // (wave-uniform)
    if (lane == 0) red_[20 + wv] = empty_w ? 1.0 : 0.0;
    LSCQP_DAS_BARRIER();
    // the four ballots in one request and one wait, combined without a branch (`||` around a load is a test around a load: four
    // dependent LDS round trips); they are adjacent and 16-byte aligned in the carve: two 16-byte words.  A ballot is 0 or 1: their
    // maximum, compared once (four comparisons joined with `|` are four scalar-register pairs, and <5,3,1,5,2> spilled 184 of them
    // against 174)
    const double2 b01 = *reinterpret_cast<const double2*>(red_ + 20), b23 = *reinterpret_cast<const double2*>(red_ + 22);
    const bool empty_g = fmax(fmax(b01.x, b01.y), fmax(b23.x, b23.y)) != 0.0;
#else
    if (tid == 0) ctl_[4] = 0.0;
    LSCQP_DAS_BARRIER();
    if (empty) ctl_[4] = 1.0;  // (benign race: every writer stores 1)
    LSCQP_DAS_BARRIER();
    const bool empty_g = ctl_[4] != 0.0;
#endif
    if (empty_g) {  // an empty interval (lo > hi on one control point: exact); its violation is the largest overlap lo - hi
        double ov = 0.0;
        if (wv == 0) {  // (the two-sided rows of the other families have lo = -hs <= hi = hs: they never raise it)
            for (int r = lane; r < NPAIR; r += 64)
                if ((pix_[r] >> 24) != 0) ov = fmax(ov, plo_[r] - phi_[r]);
            ov = wave_max(ov);
        }
        infeasible_out(0, ov);
        LSCQP_DAS_END(kDasInfeasible);
    }
    DAS_T(1);  // tables, two-sided rows, unconstrained optimum

    // ---- rows by id ---------------------------------------------------------------------------------------------------------------------
    // LSC row j, translated to the agent's position; false: the reference drops it (:404-406: first three control points, :409-411: zero normal)
    auto translate = [&](int j, double x, double y, double z, double w, double& nx, double& ny, double& nz, double& b) -> bool {
        nx = x, ny = y, nz = (dim == 3) ? z : 0.0;
        // (the whole sum per arm, not `... + (dim == 3 ? z * org2 : 0.0)`: where dim is a compile-time constant -- the fused kernel -- the compiler
        // drops the dead arm and contracts z * org2 into the sum; where it is a run-time value it could not, and the two forms of the phase differed
        // in the last bit of b on instances with active LSC rows.  Each arm below is what the fused kernel compiles for its dim: its code is unchanged.)
        b = (dim == 3) ? w - (x * org0 + y * org1 + z * org2) : w - (x * org0 + y * org1 + 0.0);
        return !(x * x + y * y + z * z < 1e-10) && (j - P * fdiv(j, iP)) >= 3;
    };
    auto load_row = [&](int j, double& nx, double& ny, double& nz, double& b) -> bool {  // (single rows: the candidate's)
        if (rows_in_lds) {  // (uniform) staged by the first pass: dropped rows hold (0, 0, 0 | -1)
            nx = Sx_[j], ny = Sy_[j], nz = Sz_[j], b = Sb_[j];
            return b != -1.0 || nx != 0.0 || ny != 0.0 || nz != 0.0;
        }
        double x, y, z, w;
        fetch_row(j, x, y, z, w);
        return translate(j, x, y, z, w, nx, ny, nz, b);
    };
    // stencil of a two-sided row on a vector in c_ layout
    // (every family as the three-point stencil v[i0] + a1 v[i1] + a2 v[e0] with loads that carry no test: a branch per family makes the
    // compiler wait for each family's loads in turn; the products with -1, -2, 1, 0 are exact, the value is the plain expression's)
    auto pair_val = [&](int pk, const double* vec) -> double {
        const int type = pk >> 24, e0 = (pk >> 12) & 0xfff, e1 = pk & 0xfff;
        const int i0 = (type == 4) ? e1 : e0 + max(type - 1, 0);  // 1: c[e0]   2: c[e0+1] - c[e0]   3: c[e0+2] - 2 c[e0+1] + c[e0]   4: c[e1] - c[e0]
        const int i1 = (type == 3) ? e0 + 1 : e0;
        const double a1 = (type <= 1) ? 0.0 : (type == 3) ? -2.0 : -1.0;
        const double a2 = (type == 3) ? 1.0 : 0.0;
        const double v0 = vec[i0], v1 = vec[i1], v2 = vec[e0];
        return (v0 + a1 * v1) + a2 * v2;
    };
    auto ent_of = [&](int e) -> int {  // position in c_ -> axis << 16 | control point
        const int k = fdiv(e, iP);
        return (k << 16) | (e - k * P);
    };
    // the row with id `rid` as entries (uniform over the workgroup)
    auto decode = [&](int rid, Row& R) {
        R.ent[0] = R.ent[1] = R.ent[2] = 0;
        R.coef[0] = R.coef[1] = R.coef[2] = 0.0;
        if (rid < nL) {
            const int cp = rid - P * fdiv(rid, iP);
            double nx, ny, nz, b;
            (void)load_row(rid, nx, ny, nz, b);
            R.ent[0] = cp, R.ent[1] = (1 << 16) | cp, R.ent[2] = (2 << 16) | cp;
            R.coef[0] = nx, R.coef[1] = ny, R.coef[2] = (dim == 3) ? nz : 0.0;
            R.rhs = b;
            return;
        }
#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
        // the stencil and BOTH bounds asked for together, at a clamped index; the side selects the bound (it chose which one to READ,
        // behind the stencil's wait: a second round trip).  (Not taken by an empty asm: that costs <5,3,1,5,2> four scalar-register
        // spills.  Without it <10,2,1,5,2>, where the id is a scalar, still waits for the stencil in front of the two bounds.)
        const int s = rid - nL, rc_ = min(s >> 1, NPAIR - 1);
        const int pk = pix_[rc_];
        const double lo_w = plo_[rc_], hi_w = phi_[rc_];
#else
        const int s = rid - nL, r = s >> 1, pk = pix_[r];
#endif
        const int type = pk >> 24, e0 = (pk >> 12) & 0xfff, e1 = pk & 0xfff;
        const double sg = (s & 1) ? -1.0 : 1.0;
#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
        R.rhs = (s & 1) ? -hi_w : lo_w;
#else
        R.rhs = (s & 1) ? -phi_[r] : plo_[r];
#endif
        // 1: c[e0]   2: c[e0+1] - c[e0]   3: c[e0+2] - 2 c[e0+1] + c[e0]   else (4): c[e1] - c[e0].  Selects, not a chain of branches: with
        // the fused kernel's compile-time carve, the compiler merged the branches so that a pair row (type 4) left the phase with coef[1]
        // undefined (0 in practice) -- a different row, found on c1_infeasible_1pct (NOTES.md section 16).  The values are the branches' own.
        const bool t1 = type == 1, t2 = type == 2, t3 = type == 3;
        R.ent[0] = ent_of(t1 ? e0 : t2 ? e0 + 1 : t3 ? e0 + 2 : e1);
        R.ent[1] = t1 ? 0 : ent_of(t3 ? e0 + 1 : e0);
        R.ent[2] = t3 ? ent_of(e0) : 0;
        R.coef[0] = sg;
        R.coef[1] = t1 ? 0.0 : t3 ? -2.0 * sg : -sg;
        R.coef[2] = t3 ? sg : 0.0;
    };
    auto row_dot = [&](const int* ent, const double* coef, const double* vec) -> double {  // a'vec for a vector in c_ layout
        return coef[0] * vec[ent_axis(ent[0]) * P + ent_cp(ent[0])] + coef[1] * vec[ent_axis(ent[1]) * P + ent_cp(ent[1])] +
               coef[2] * vec[ent_axis(ent[2]) * P + ent_cp(ent[2])];
    };

    // ---- one pass over every row: the most violated one (RAW slack, lowest id on ties); its slack is the largest raw violation -------
    // The FIRST pass consumes the rows requested in the prologue (HBM), asks for the rest four at a time and, in the staged form (small
    // batches: LDS to spare), leaves them translated in LDS; later passes read them from there, or from L2.
    bool first_pass = true;  // (uniform)
#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
    // This thread's LSC rows stay in registers across the loop of steps: row tid + u T is this thread's in every pass, the first pass
    // translated it (dropped rows and slots past the end neutralised to (0, 0, 0 | -1)) and stored it to the staged arrays, and a later
    // pass read back what the same thread had written.  With them the control point of each slot: where the row's operands stand in c_.
    // The staged arrays keep their stores -- decode and the infeasibility proof read the candidate's row from there.
    // They are translated HERE, in front of the loop of steps and not inside the first pass: nothing in the loop then writes them, and
    // they are not carried around it through copies.  (prep's text; the rows from memory are waited for where the first pass did.)
    double kx_[kU], ky_[kU], kz_[kU], kb_[kU];
    int kcp_[kU];
#pragma unroll
    for (int u = 0; u < kU; u++) {
        const int j = tid + u * T, jc = j < nL ? j : 0;
        const bool ok = translate(jc, px[u], py[u], pz[u], pw[u], kx_[u], ky_[u], kz_[u], kb_[u]) && j < nL;
        kx_[u] = ok ? kx_[u] : 0.0, ky_[u] = ok ? ky_[u] : 0.0, kz_[u] = ok ? kz_[u] : 0.0, kb_[u] = ok ? kb_[u] : -1.0;
        kcp_[u] = jc - P * fdiv(jc, iP);
    }
#endif
    // Rows are judged by their RAW slack (metres, the interior-point kernel's bar), which is also what picks the candidate.  Straight-line code:
    // a dropped row, or a slot behind the instance's last row, is the harmless row (0, 0, 0 | -1) -- slack +1 -- instead of a branch.
    auto pass_local = [&](double& bv, int& bi) {
        bv = 1e300;
        bi = 0x7fffffff;
        auto see = [&](double slack, int id) {
            // (a NaN slack -- NaN in a row, in the header, in the point -- must never read as "satisfied": it becomes the most violated row
            // there is; the step for it finds no length and the instance goes to the interior-point kernel, which answers NUMERIC)
            slack = (slack == slack) ? slack : -1e308;
            const bool lt = slack < bv;  // (ids ascend within a thread: the first minimum is the lowest id)
            bv = lt ? slack : bv;
            bi = lt ? id : bi;
        };
        auto eval = [&](int j0, const double* rx, const double* ry, const double* rz, const double* rb) {
#pragma unroll
            for (int u = 0; u < kU; u++) {
                const int j = j0 + u * T, jc = j < nL ? j : 0;
                const int cp = jc - P * fdiv(jc, iP);
                see(rx[u] * c_[cp] + ry[u] * c_[P + cp] + rz[u] * c_[2 * P + cp] - rb[u], j);
            }
        };
        // raw -> translated, dropped rows and slots past the end neutralised
        auto prep = [&](int j0, const double* x, const double* y, const double* z, const double* w, double* rx, double* ry, double* rz, double* rb) {
#pragma unroll
            for (int u = 0; u < kU; u++) {
                const int j = j0 + u * T, jc = j < nL ? j : 0;
                const bool ok = translate(jc, x[u], y[u], z[u], w[u], rx[u], ry[u], rz[u], rb[u]) && j < nL;
                rx[u] = ok ? rx[u] : 0.0, ry[u] = ok ? ry[u] : 0.0, rz[u] = ok ? rz[u] : 0.0, rb[u] = ok ? rb[u] : -1.0;
            }
        };
        auto stage = [&](int j0, const double* rx, const double* ry, const double* rz, const double* rb) {
#pragma unroll
            for (int u = 0; u < kU; u++) {
                const int j = j0 + u * T;
                if (j < nL) Sx_[j] = rx[u], Sy_[j] = ry[u], Sz_[j] = rz[u], Sb_[j] = rb[u];
            }
        };
#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
        const double* const rx = kx_, * const ry = ky_, * const rz = kz_, * const rb = kb_;  // (the thread's rows, translated above)
        // the two-sided rows of this thread from the registers the prologue left (tp_*): the pass reads nothing of pix_ / plo_ / phi_, only
        // the stencils' operands in c_, and asks for those where `ts_request` stands
        double tv0[kPR], tv1[kPR], tv2[kPR];
        bool ts_asked = false;  // (a constant after inlining)
        auto ts_request = [&]() {
#pragma unroll
            for (int u = 0; u < kPR; u++) tv0[u] = c_[tp_i0[u]], tv1[u] = c_[tp_i1[u]], tv2[u] = c_[tp_e0[u]];
            ts_asked = true;
        };
        auto ts_see = [&]() {
#pragma unroll
            for (int u = 0; u < kPR; u++) {
                const int r = tid + u * T;
                const double d = (tv0[u] + tp_a1[u] * tv1[u]) + tp_a2[u] * tv2[u];  // (pair_val's expression)
                const bool on = (tp_pk[u] >> 24) != 0;
                see(on ? d - tp_lo[u] : 1.0, nL + 2 * r);
                see(on ? tp_hi[u] - d : 1.0, nL + 2 * r + 1);
            }
        };
#else
        double rx[kU], ry[kU], rz[kU], rb[kU];
#endif
        if (first_pass) {
#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
            // The first pass in ONE block of requests, as the later pass: the operands in c_ of the thread's LSC rows and of its two-sided
            // rows (the translation above needs the rows from memory and the origin, nothing else of LDS); the staging stores are issued
            // behind the requests, the slacks are eval's expression in eval's slot order.  One block of row slots holds every row of the
            // shape: no further trip.
            double cx[kU], cy[kU], cz[kU];
#pragma unroll
            for (int u = 0; u < kU; u++) {
                const int cp = kcp_[u];
                cx[u] = c_[cp], cy[u] = c_[P + cp], cz[u] = c_[2 * P + cp];
            }
            ts_request();
            __builtin_amdgcn_sched_barrier(0);  // (every request above stands in front of the first use below)
            if (staged) stage(tid, rx, ry, rz, rb);
#pragma unroll
            for (int u = 0; u < kU; u++) see(rx[u] * cx[u] + ry[u] * cy[u] + rz[u] * cz[u] - rb[u], tid + u * T);  // (eval's expression)
#else
            // the prologue's rows, then the rest from memory
            prep(tid, px, py, pz, pw, rx, ry, rz, rb);
            if (staged) stage(tid, rx, ry, rz, rb);
            eval(tid, rx, ry, rz, rb);
            for (int j0 = tid + kU * T; kMaxNL > kU * T && j0 < nL; j0 += kU * T) {  // (no trip where the class's rows fit one block)
                double x[kU], y[kU], z[kU], w[kU];
#pragma unroll
                for (int u = 0; u < kU; u++) fetch_row(j0 + u * T < nL ? j0 + u * T : 0, x[u], y[u], z[u], w[u]);
                prep(j0, x, y, z, w, rx, ry, rz, rb);
                if (staged) stage(j0, rx, ry, rz, rb);
                eval(j0, rx, ry, rz, rb);
            }
#endif
        } else if (rows_in_lds) {
#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
            // The later pass reads NO staged row: the thread's rows are the registers the first pass stored to the staged arrays from (and
            // the harmless row in a slot past the end -- the values the other text's reads give).  ONE block of requests: the rows'
            // operands in c_ and the two-sided rows'.
            double cx[kU], cy[kU], cz[kU];
#pragma unroll
            for (int u = 0; u < kU; u++) cx[u] = c_[kcp_[u]], cy[u] = c_[P + kcp_[u]], cz[u] = c_[2 * P + kcp_[u]];
            ts_request();
            __builtin_amdgcn_sched_barrier(0);  // (every request above stands in front of the first use below)
#pragma unroll
            for (int u = 0; u < kU; u++) see(rx[u] * cx[u] + ry[u] * cy[u] + rz[u] * cz[u] - rb[u], tid + u * T);  // (eval's expression)
#else
            for (int j0 = tid; j0 < nL; j0 += kU * T) {
#pragma unroll
                for (int u = 0; u < kU; u++) {
                    const int j = j0 + u * T, jc = j < nL ? j : 0;
                    rx[u] = Sx_[jc], ry[u] = Sy_[jc], rz[u] = Sz_[jc], rb[u] = (j < nL) ? Sb_[jc] : 1e300;  // (a slot past the end: slack -> -inf guard below)
                    if (!(j < nL)) rx[u] = ry[u] = rz[u] = 0.0, rb[u] = -1.0;
                }
                eval(j0, rx, ry, rz, rb);
            }
#endif
        } else {
            for (int j0 = tid; j0 < nL; j0 += kU * T) {
                double x[kU], y[kU], z[kU], w[kU];
#pragma unroll
                for (int u = 0; u < kU; u++) fetch_row(j0 + u * T < nL ? j0 + u * T : 0, x[u], y[u], z[u], w[u]);
#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
                double nx_[kU], ny_[kU], nz_[kU], nb_[kU];  // (rows that are not staged: translated again in every pass, as they were)
                prep(j0, x, y, z, w, nx_, ny_, nz_, nb_);
                eval(j0, nx_, ny_, nz_, nb_);
#else
                prep(j0, x, y, z, w, rx, ry, rz, rb);
                eval(j0, rx, ry, rz, rb);
#endif
            }
        }
        first_pass = false;
        DAS_T(8);
#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
        if (!ts_asked) ts_request();  // (a pass over rows that are not staged)
        ts_see();
#else
        for (int r0 = tid; r0 < NPAIR; r0 += 2 * T) {  // two at a time: their LDS round trips overlap
            const int r1 = r0 + T, r1c = r1 < NPAIR ? r1 : r0;
            const int pk0 = pix_[r0], pk1 = pix_[r1c];
            const double lo0 = plo_[r0], hi0 = phi_[r0], lo1 = plo_[r1c], hi1 = phi_[r1c];
            const double d0 = pair_val(pk0, c_), d1 = pair_val(pk1, c_);
            const bool on0 = (pk0 >> 24) != 0, on1 = (pk1 >> 24) != 0 && r1 < NPAIR;
            see(on0 ? d0 - lo0 : 1.0, nL + 2 * r0);
            see(on0 ? hi0 - d0 : 1.0, nL + 2 * r0 + 1);
            see(on1 ? d1 - lo1 : 1.0, nL + 2 * r1);
            see(on1 ? hi1 - d1 : 1.0, nL + 2 * r1 + 1);
        }
#endif
        DAS_T(9);
    };
    // the workgroup's (slack, id) minimum out of the wavefronts' (buffer rb_: values at [0, 4), ids as ints at [4, 6))
    auto pass_combine = [&](const double* rb_, double& bv, int& bi) {
#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
        // the four values and the four ids in one request and one wait (three 16-byte words: the buffer is 16-byte aligned), the lexicographic
        // minimum by selects in the loop's order: `||` and `&&` around the loads made three to four dependent LDS round trips and six
        // branches of it
        const double2 v01 = *reinterpret_cast<const double2*>(rb_), v23 = *reinterpret_cast<const double2*>(rb_ + 2);
        const int4 ids = *reinterpret_cast<const int4*>(rb_ + 4);
        const double ovs[4] = {v01.x, v01.y, v23.x, v23.y};
        const int ois[4] = {ids.x, ids.y, ids.z, ids.w};
        bv = ovs[0], bi = ois[0];
#pragma unroll
        for (int w = 1; w < NW; w++) {
            const bool lt = (ovs[w] < bv) | ((ovs[w] == bv) & (ois[w] < bi));
            bv = lt ? ovs[w] : bv, bi = lt ? ois[w] : bi;
        }
#else
        bv = rb_[0], bi = reinterpret_cast<const int*>(rb_ + 4)[0];
#pragma unroll
        for (int w = 1; w < NW; w++) {
            const double ov = rb_[w];
            const int oi = reinterpret_cast<const int*>(rb_ + 4)[w];
            if (ov < bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
        }
#endif
    };
    auto pass = [&](double& best, int& bid) {
        const bool was_first = first_pass;
        double bv;
        int bi;
        pass_local(bv, bi);
        if constexpr (kTableEarly) {  // (the latency text, where the table fits the registers)
            if (was_first) {  // the class's table, from the registers the prologue asked for; the barrier below publishes it
#pragma unroll
                for (int i = 0; i < kCPre; i++) {
                    const int e = tid + i * T;
                    if (e < P * P) Cc_[e] = cpre[i];
                }
            }
        }
        DAS_ARGMIN(bv, bi);
        if constexpr (NW > 1) {
            double* const rb_ = red_ + 24 * par;
            par ^= 1;
            if (lane == 0) {
                rb_[wv] = bv;
                reinterpret_cast<int*>(rb_ + 4)[wv] = bi;
            }
            LSCQP_DAS_BARRIER();
            pass_combine(rb_, bv, bi);
        } else if (staged && was_first) {
            LSCQP_DAS_BARRIER();  // the staged rows are read by other lanes from now on
        }
        if (staged) rows_in_lds = true;
        best = bv, bid = bi;
    };

    // ---- the small factor: S = A'C A (k x k, SPD), S = Lm Lm', rows owned by the lanes of wavefront 0 -------------------------------------
    const double* Cm = kTableEarly ? Cc_ : Cg;  // column cp = Cm + cp * P (symmetric); the LDS copy once a step needs it (or from the first pass on)
    // The small system S = A'C A of the active rows is carried as J = L^-1, the INVERSE of its Cholesky factor (lower triangular, zeros kept
    // above the diagonal): S^-1 = J'J, so r = S^-1 v is two matrix-vector products without a dependent chain (a substitution through L is
    // 2k dependent broadcast-multiply-subtract steps), a joining row appends the row (-r' , 1) / sqrt(a_p'w_p - v'r) -- r is this step's --
    // and a leaving row costs k - l rotations of row pairs.  Lane i of wavefront 0 = row i (products) / column i (rotations).
    //
    // Row l leaves: rotations of the rows (l, l + 1), (l + 1, l + 2), ... push column l's content into the last row, which is dropped with
    // the column (Goldfarb-Idnani's downdate on J).  In place: the lane of column c writes column c - [c > l] of row j after every lane
    // has read rows j and j + 1 (LDS operations of one wavefront execute in order).  false on a vanishing pivot.
    auto factor_remove = [&](int k_, int l_) -> bool {
        bool ok = true;
        if (wv == 0) {
            const int k = __builtin_amdgcn_readfirstlane(k_), l = __builtin_amdgcn_readfirstlane(l_);
            const bool mine = lane < k;
            const int c = mine ? lane : 0;
            const int cn = c - (c > l ? 1 : 0);
            double carry = Jm_[l * LDL + c];
            double a = Jm_[l * LDL + l];
            for (int j = l; j < k - 1; j++) {
                const double x = Jm_[(j + 1) * LDL + c];
                const double b = Jm_[(j + 1) * LDL + l];
                const double r2 = a * a + b * b;
                if (!(r2 > 1e-280)) ok = false;
                const double ir = rsqrt(fmax(r2, 1e-300));
                const double ca = a * ir, sb = b * ir;
                const double fin = ca * x - sb * carry;  // the new row j: nothing left in column l, a positive diagonal
                carry = ca * carry + sb * x;
                a = r2 * ir;
                if (mine && lane != l) Jm_[j * LDL + cn] = fin;
            }
            if (mine) Jm_[(k - 1) * LDL + lane] = 0.0, Jm_[lane * LDL + k - 1] = 0.0;  // (J is zero outside its k x k block: solve_factor reads windows)
            LSCQP_DAS_WAVE_SYNC();
        }
        return ok;
    };
    // r = S^-1 v = J'(J v) (wavefront 0; lane j holds v_j on entry and r_j on return, also left in r_; yy = v'S^-1 v = |J v|^2 if asked for).
    // The factor's entries are requested a window of eight columns ahead so that no LDS round trip sits between the multiply-adds; the
    // loads carry no condition (J is zero outside its block, the index is clamped into the array): a test around a load makes the compiler
    // wait for each one in turn.
    auto solve_factor = [&](int k_, double vi, double* yy) -> double {
        const int k = __builtin_amdgcn_readfirstlane(k_);
        const bool mine = lane < k;
        const int ll = min(lane, kcap - 1);
        vi = mine ? vi : 0.0;
        double yi = 0.0, ri = 0.0;
        for (int j0 = 0; j0 < k; j0 += 8) {  // y = J v (row ll of J)
            double Jr[8];
#pragma unroll
            for (int t_ = 0; t_ < 8; t_++) Jr[t_] = Jm_[ll * LDL + min(j0 + t_, kcap)];  // (column kcap: always zero)
#pragma unroll
            for (int t_ = 0; t_ < 8; t_++) yi += Jr[t_] * lscqp::bcast(vi, j0 + t_);  // (k <= 32: the lane index stays below 64; lanes >= k hold 0)
        }
        yi = mine ? yi : 0.0;
        if (yy) *yy = DAS_SUM(yi * yi);
        for (int j0 = 0; j0 < k; j0 += 8) {  // r = J'y (column ll of J)
            double Jc[8];
#pragma unroll
            for (int t_ = 0; t_ < 8; t_++) Jc[t_] = Jm_[min(j0 + t_, kcap - 1) * LDL + ll];  // (a clamped row meets y = 0)
#pragma unroll
            for (int t_ = 0; t_ < 8; t_++) ri += Jc[t_] * lscqp::bcast(yi, j0 + t_);
        }
        ri = mine ? ri : 0.0;
        if (lane < kcap + 4) r_[lane] = ri;  // (zeros behind the active rows: the update of c reads a window of four without a test)
        return ri;
    };
    // c_[e] = base[e] (or c_[e]) + sum_j wts[j] W_j[e] over the active rows
    auto add_columns = [&](int k, const double* wts, const double* base) {
        for (int e = tid; e < NX; e += T) {
            double a = base ? base[e] : c_[e];
            for (int j = 0; j < k; j++) a += wts[j] * W_[(size_t)j * NX + e];
            c_[e] = a;
        }
    };

    // ---- verification + objective, one reduction: reduced stationarity T'(Hx c + fx - A'u) scaled as lscqp_info.res_dual; objective exactly
    // as cplex.getObjValue() reports it (as lscqp_kernel.hpp).  Every z thread evaluates the <= 4 control-point rows of Hx it needs itself.
    const int NZA = 3 * (M - 1) + (es ? 1 : 3);
    auto finish_local = [&](int k, double& rd, double& gs, double& part) {
#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
        // (the class's, left in LDS by the prologue; the two ka_ names stand in front of the block's registers for DAS_CLS below)
        const double dt = wb_[6], q2s = wb_[7], ka_w_t = ctl_[4], ka_w_c = red_[44], wt2 = 2.0 * ka_w_t;
        // The same verification as straight-line code (the expressions that round are the other text's below, word for word): every operand
        // of a stationarity lane -- header words, origin, the twelve words of c_ of its segment and the next -- is asked for before the
        // first arithmetic, at clamped indices and without a test around a load (a lane past the last row evaluates the last row, a last
        // segment evaluates itself as its "next" one; their values are dropped by selects).  lam_ is read as it stands: the prologue
        // zeroed it, thread 0 adds A'u to the zeros, so no zeroing pass and no barrier of its own stand in front of thread 0's sums.
        // the objective's part of this thread, from one block of loads
        auto objective_local = [&]() {
            // One wavefront (the second), straight-line: the lane's six control points, the 36 words of the rounding term, origin and goal
            // are all asked for in front of the first arithmetic (the other text's row-at-a-time loop is six dependent LDS round trips);
            // the sums in the loop's order.  (a lane without a segment evaluates the last one and its value is dropped)
            part = 0.0;
            if (__builtin_amdgcn_readfirstlane(wv) == 1) {
                const bool on = lane < dim * M;
                const int lv = on ? lane : dim * M - 1;
                const int kx = lv / M, m = lv - kx * M;
                const double* cc = &c_[kx * P + 6 * m];
                double cv[6], dqv[36];
                double ok_ = org[kx], gl_ = Hd->goal[kx];
#pragma unroll
                for (int i = 0; i < 6; i++) cv[i] = cc[i];
#pragma unroll
                for (int i = 0; i < 36; i++) dqv[i] = dq_[i];
                asm volatile("" : "+v"(ok_), "+v"(gl_));
#pragma unroll
                for (int i = 0; i < 6; i++) asm volatile("" : "+v"(cv[i]));
#pragma unroll
                for (int i = 0; i < 36; i++) asm volatile("" : "+v"(dqv[i]));
                const double j0 = (cv[3] - cv[0]) - 3.0 * (cv[2] - cv[1]);
                const double j1 = (cv[4] - cv[1]) - 3.0 * (cv[3] - cv[2]);
                const double j2 = (cv[5] - cv[2]) - 3.0 * (cv[4] - cv[3]);
                const double quad = 0.2 * (j0 * j0 + j2 * j2) + (2.0 / 15.0) * j1 * j1 + 0.2 * (j0 * j1 + j1 * j2) + (1.0 / 15.0) * j0 * j2;
                double pp = 0.5 * q2s * 3600.0 * quad;
                double corr = 0;
                const double s0 = cv[0] + ok_, s1 = cv[1] + ok_, s2 = cv[2] + ok_, s3 = cv[3] + ok_, s4 = cv[4] + ok_, s5 = cv[5] + ok_;
#pragma unroll
                for (int i = 0; i < 6; i++) {
                    const double* dr = dqv + 6 * i;
                    double r = 0;
                    r += dr[0] * s0, r += dr[1] * s1, r += dr[2] * s2, r += dr[3] * s3, r += dr[4] * s4, r += dr[5] * s5;
                    corr += r * (cv[i] + ok_);
                }
                pp += DAS_CLS(w_c) * corr;
                const double dgoal = cv[5] - (gl_ - ok_);
                pp += (m >= M - ts) ? DAS_CLS(w_t) * dgoal * dgoal : 0.0;
                const double sum = part + pp;
                part = on ? sum : part;
            }
        };
        const int nz = dim * NZA;  // (<= 108 < T)
        const bool zw = __builtin_amdgcn_readfirstlane(wv) * 64 < nz;  // (wave-uniform: a wavefront without a row skips the section)
        const bool zon = tid < nz;
        const int zi = zon ? tid : nz - 1;
        const int kx = zi / NZA, a = zi - kx * NZA;
        const bool last = es && a == 3 * (M - 1);
        const int m = last ? M - 1 : a / 3, j = last ? 0 : a % 3;
        const bool has_next = m + 1 < M;
        const int mn = has_next ? m + 1 : M - 1;
        double hv0, ha0, hgl, hok, va[6], vb[6];
        if (zw) {
            hv0 = Hd->v0[kx], ha0 = Hd->a0[kx], hgl = Hd->goal[kx], hok = org[kx];
#pragma unroll
            for (int i = 0; i < 6; i++) va[i] = c_[kx * P + 6 * m + i], vb[i] = c_[kx * P + 6 * mn + i];
        }
        if (k > 0) {  // A'u, per control point, onto the zeros
            if (tid == 0) {
                for (int j_ = 0; j_ < k; j_++)
#pragma unroll
                    for (int t_ = 0; t_ < 3; t_++) {
                        const int en = aint_[4 * j_ + 1 + t_];
                        lam_[ent_axis(en) * P + ent_cp(en)] += u_[j_] * acoef_[3 * j_ + t_];
                    }
            }
            LSCQP_DAS_BARRIER();
        }
        objective_local();  // (behind the barrier, beside the stationarity rows: in front of it, beside thread 0's sums, the slot timed the same)
        rd = 0.0, gs = 0.0;
        if (zw) {
            double la[3], lb[3];
#pragma unroll
            for (int i = 0; i < 3; i++) la[i] = lam_[kx * P + 6 * m + 3 + i], lb[i] = lam_[kx * P + 6 * mn + i];
            double dt_ = dt, q2s_ = q2s, wt2_ = wt2;
            asm volatile("" : "+v"(hv0), "+v"(ha0), "+v"(hgl), "+v"(hok), "+v"(dt_), "+v"(q2s_), "+v"(wt2_));
#pragma unroll
            for (int i = 0; i < 6; i++) asm volatile("" : "+v"(va[i]), "+v"(vb[i]));
#pragma unroll
            for (int i = 0; i < 3; i++) asm volatile("" : "+v"(la[i]), "+v"(lb[i]));
            {
                const double dt = dt_, q2s = q2s_, wt2 = wt2_;
                const double c1 = hv0 * dt * 0.2;
                const double c2 = ha0 * dt * dt * 0.05 + 2.0 * c1;
                const double gk = hgl - hok;
                // the six rows of Hx of one segment on this axis: g = Hx c + fx, g0 = Hx cfix + fx (constant indices: registers)
                auto seg = [&](int mm, const double* cc, double* g, double* g0) {
                    const double v0 = cc[0], v1 = cc[1], v2 = cc[2], v3 = cc[3], v4 = cc[4], v5 = cc[5];
                    lscqp::static_for<0, 6>([&](auto Ic) {
                        constexpr int i = decltype(Ic)::value;
                        g[i] = q2s * (KQ(i, 0) * v0 + KQ(i, 1) * v1 + KQ(i, 2) * v2 + KQ(i, 3) * v3 + KQ(i, 4) * v4 + KQ(i, 5) * v5);
                        g0[i] = (mm == 0) ? q2s * (KQ(i, 1) * c1 + KQ(i, 2) * c2) : 0.0;
                    });
                    if (mm >= M - ts) {
                        g[5] += wt2 * (v5 - gk);
                        g0[5] += -wt2 * gk;
                    }
                };
                double g[6], g0[6];
                seg(m, va, g, g0);
                const double lm3 = la[0], lm4 = la[1], lm5 = la[2];  // A'u on the segment's last three control points
                double cf, cg, c0;  // T' of: full residual, gradient, gradient at the fixed part
                {
                    const double cf_l = (g[3] - lm3) + (g[4] - lm4) + (g[5] - lm5), cg_l = g[3] + g[4] + g[5], c0_l = g0[3] + g0[4] + g0[5];
                    const double gs_ = j == 0 ? g[3] : j == 1 ? g[4] : g[5], ls_ = j == 0 ? lm3 : j == 1 ? lm4 : lm5, g0s = j == 0 ? g0[3] : j == 1 ? g0[4] : g0[5];
                    cf = last ? cf_l : gs_ - ls_, cg = last ? cg_l : gs_, c0 = last ? c0_l : g0s;
                }
                {  // (c0, c1, c2) of the next segment = TB (c3, c4, c5) of this one, TB = [[0,0,1],[0,-1,2],[1,-4,4]]
                    seg(mn, vb, g, g0);
                    const double* const lm = lb;
                    const double w0 = (j == 2) ? 1.0 : 0.0, w1 = (j == 1) ? -1.0 : (j == 2) ? 2.0 : 0.0, w2 = (j == 0) ? 1.0 : (j == 1) ? -4.0 : 4.0;
                    const double cf_n = cf + (w0 * (g[0] - lm[0]) + w1 * (g[1] - lm[1]) + w2 * (g[2] - lm[2]));
                    const double cg_n = cg + (w0 * g[0] + w1 * g[1] + w2 * g[2]);
                    const double c0_n = c0 + (w0 * g0[0] + w1 * g0[1] + w2 * g0[2]);
                    cf = has_next ? cf_n : cf, cg = has_next ? cg_n : cg, c0 = has_next ? c0_n : c0;
                }
                const double rd_ = fmax(rd, fabs(cf)), gs_z = fmax(gs, fmax(fabs(cg), fabs(c0)));
                rd = zon ? rd_ : rd, gs = zon ? gs_z : gs;
            }
        }
#else
        if (k > 0) {  // A'u, per control point
            for (int e = tid; e < NX; e += T) lam_[e] = 0.0;
            LSCQP_DAS_BARRIER();
            if (tid == 0) {
                for (int j = 0; j < k; j++)
#pragma unroll
                    for (int t_ = 0; t_ < 3; t_++) {
                        const int en = aint_[4 * j + 1 + t_];
                        lam_[ent_axis(en) * P + ent_cp(en)] += u_[j] * acoef_[3 * j + t_];
                    }
            }
            LSCQP_DAS_BARRIER();
        }
        rd = 0.0, gs = 0.0;
        for (int zi = tid; zi < dim * NZA; zi += T) {
            const int kx = zi / NZA, a = zi - kx * NZA;
            const bool last = es && a == 3 * (M - 1);
            const int m = last ? M - 1 : a / 3, j = last ? 0 : a % 3;
            const double c1 = Hd->v0[kx] * dt * 0.2;
            const double c2 = Hd->a0[kx] * dt * dt * 0.05 + 2.0 * c1;
            const double gk = Hd->goal[kx] - org[kx];
            // the six rows of Hx of one segment on this axis: g = Hx c + fx, g0 = Hx cfix + fx, lm = A'u (constant indices: registers)
            auto seg = [&](int mm, double* g, double* g0, double* lm) {
                const double* cc = &c_[kx * P + 6 * mm];
                const double v0 = cc[0], v1 = cc[1], v2 = cc[2], v3 = cc[3], v4 = cc[4], v5 = cc[5];
                lscqp::static_for<0, 6>([&](auto Ic) {
                    constexpr int i = decltype(Ic)::value;
                    g[i] = q2s * (KQ(i, 0) * v0 + KQ(i, 1) * v1 + KQ(i, 2) * v2 + KQ(i, 3) * v3 + KQ(i, 4) * v4 + KQ(i, 5) * v5);
                    g0[i] = (mm == 0) ? q2s * (KQ(i, 1) * c1 + KQ(i, 2) * c2) : 0.0;
                    lm[i] = (k > 0) ? lam_[kx * P + 6 * mm + i] : 0.0;
                });
                if (mm >= M - ts) {
                    g[5] += wt2 * (v5 - gk);
                    g0[5] += -wt2 * gk;
                }
            };
            double g[6], g0[6], lm[6];
            seg(m, g, g0, lm);
            double cf, cg, c0;  // T' of: full residual, gradient, gradient at the fixed part
            if (last) {
                cf = (g[3] - lm[3]) + (g[4] - lm[4]) + (g[5] - lm[5]), cg = g[3] + g[4] + g[5], c0 = g0[3] + g0[4] + g0[5];
            } else {
                const double gs_ = j == 0 ? g[3] : j == 1 ? g[4] : g[5], ls_ = j == 0 ? lm[3] : j == 1 ? lm[4] : lm[5], g0s = j == 0 ? g0[3] : j == 1 ? g0[4] : g0[5];
                cf = gs_ - ls_, cg = gs_, c0 = g0s;
            }
            if (m + 1 < M) {  // (c0, c1, c2) of the next segment = TB (c3, c4, c5) of this one, TB = [[0,0,1],[0,-1,2],[1,-4,4]]
                seg(m + 1, g, g0, lm);
                const double w0 = (j == 2) ? 1.0 : 0.0, w1 = (j == 1) ? -1.0 : (j == 2) ? 2.0 : 0.0, w2 = (j == 0) ? 1.0 : (j == 1) ? -4.0 : 4.0;
                cf += w0 * (g[0] - lm[0]) + w1 * (g[1] - lm[1]) + w2 * (g[2] - lm[2]);
                cg += w0 * g[0] + w1 * g[1] + w2 * g[2];
                c0 += w0 * g0[0] + w1 * g0[1] + w2 * g0[2];
            }
            rd = fmax(rd, fabs(cf));
            gs = fmax(gs, fmax(fabs(cg), fabs(c0)));
        }
        part = 0.0;
        // (the objective's threads sit in the second wavefront when there is one: its arithmetic runs beside the stationarity rows' instead of behind them)
        for (int lv = tid - (NW > 1 ? 64 : 0); lv < dim * M; lv += T) {
            if (lv < 0) continue;
            const int kx = lv / M, m = lv - kx * M;
            const double* cc = &c_[kx * P + 6 * m];
            const double j0 = (cc[3] - cc[0]) - 3.0 * (cc[2] - cc[1]);
            const double j1 = (cc[4] - cc[1]) - 3.0 * (cc[3] - cc[2]);
            const double j2 = (cc[5] - cc[2]) - 3.0 * (cc[4] - cc[3]);
            const double quad = 0.2 * (j0 * j0 + j2 * j2) + (2.0 / 15.0) * j1 * j1 + 0.2 * (j0 * j1 + j1 * j2) + (1.0 / 15.0) * j0 * j2;
            double pp = 0.5 * q2s * 3600.0 * quad;
            const double ok_ = org[kx];
            double corr = 0;
            const double s0 = cc[0] + ok_, s1 = cc[1] + ok_, s2 = cc[2] + ok_, s3 = cc[3] + ok_, s4 = cc[4] + ok_, s5 = cc[5] + ok_;
#pragma unroll 1
            for (int i = 0; i < 6; i++) {  // (a row of the term at a time: unrolled, its 36 entries would be requested -- and held in registers -- at once)
                const double* dr = dq_ + 6 * i;
                double r = 0;
                r += dr[0] * s0, r += dr[1] * s1, r += dr[2] * s2, r += dr[3] * s3, r += dr[4] * s4, r += dr[5] * s5;
                corr += r * (cc[i] + ok_);
            }
            pp += DAS_CLS(w_c) * corr;
            const double dgoal = cc[5] - (Hd->goal[kx] - ok_);
            pp += (m >= M - ts) ? DAS_CLS(w_t) * dgoal * dgoal : 0.0;
            part += pp;
        }
#endif
    };
    // (buffer rb_: the wavefronts' stationarity maxima at [8, 12), gradient scales at [12, 16), objective parts at [16, 20))
    auto finish_combine = [&](const double* rb_, double& rd, double& gs, double& part) {
        rd = rb_[8], gs = rb_[12], part = rb_[16];
#pragma unroll
        for (int w = 1; w < NW; w++) rd = fmax(rd, rb_[8 + w]), gs = fmax(gs, rb_[12 + w]), part += rb_[16 + w];  // (fixed order: reproducible)
    };
    auto finish_verdict = [&](double rd, double gs, double part, double& res_d, double& obj) {
        res_d = (part == part && fabs(part) < 1e300) ? rd / fmax(1.0, gs) : 1e300;  // (a non-finite objective is not a pass)
        obj = part;
    };
    auto finish = [&](int k, double& res_d, double& obj) {
        double rd, gs, part;
        finish_local(k, rd, gs, part);
        DAS_MAX0_MAX0_SUM(rd, gs, part);  // (rd and gs are maxima of absolute values over 0.0)
        if constexpr (NW > 1) {
            double* const rb_ = red_ + 24 * par;
            par ^= 1;
            if (lane == 0) rb_[8 + wv] = rd, rb_[12 + wv] = gs, rb_[16 + wv] = part;
            LSCQP_DAS_BARRIER();
            finish_combine(rb_, rd, gs, part);
        }
        finish_verdict(rd, gs, part, res_d, obj);
    };

    // ---- the loop ---------------------------------------------------------------------------------------------------------------------
    int k = 0, steps = 0, why = LSCQP_DAS_WHY_VERIFICATION;
    bool polished = false, solved = false, haveC = false, haveJ = false, proven = false;
    double res_p = 0.0, res_d = 0.0, obj = 0.0;
    // the result: control points in the world frame
    auto write_out = [&]() {
        for (int e = tid; e < NX; e += T) x_out[q * NX + e] = c_[e] + org[fdiv(e, iP)];
        if (tid == 0) {
            obj_out[q] = obj;
            status_out[q] = LSCQP_STATUS_OPTIMAL;
            if (info_out) {
                info_out[q].iterations = steps;
                info_out[q].flags = LSCQP_INFO_ACTIVE_SET;
                info_out[q].res_primal = res_p;
                info_out[q].res_dual = res_d;
                info_out[q].gap = 0.0;  // complementarity is exact: a row is either in the set (slack 0) or carries no multiplier
            }
        }
    };
    // PEEL (batches beyond two workgroups per CU; the lean form): the first look stands in front of the loop of steps and a quiet instance
    // leaves the kernel from it.  What the loop keeps invariant -- addresses, reciprocals, spilled scalars: some 360 instructions of code a
    // quiet instance never reaches -- the compiler prepares in front of the loop, and with the first look inside the loop in front of that
    // too: 4096 quiet instances run 4 % faster peeled, 1024 x M10 x 40 4.5 %.  Not for the small batches: there ONE instance with a step
    // sets the launch's time, and it runs 2.5 % faster when the pass and the verification it repeats are the code it has just run.
    double best;
    int bid;
    bool peeled = false;
    if constexpr (PEEL || SCREEN) {
        pass(best, bid);
        DAS_T(2);  // first pass
        if (!(best < -kTolP)) {
            res_p = fmax(0.0, -best);
            finish(0, res_d, obj);
            DAS_T(4);  // verification + objective
            if (res_d <= kTolD) write_out();
            else hand_over(0, LSCQP_DAS_WHY_VERIFICATION);  // (the tables' rounding, never seen; the interior-point kernel solves the instance)
            DAS_T(7);  // epilogue
            DAS_T_FLUSH();
            LSCQP_DAS_END(res_d <= kTolD ? kDasSolved : kDasHandedOver);
        }
        peeled = true;
    }
    for (;;) {
        if (!((PEEL || SCREEN) && peeled)) {  // (the peeled forms come with their first look taken)
            pass(best, bid);
            DAS_T(steps == 0 ? 2 : 3);  // first pass / later passes
        }
        peeled = false;
        if (!(best < -kTolP)) {
            res_p = fmax(0.0, -best);
            finish(k, res_d, obj);
            DAS_T(4);  // verification + objective
            if (res_d <= kTolD) {
                solved = true;
                break;
            }
            if (polished || k == 0) break;  // (never seen on the bench's classes; the interior-point kernel then solves the instance)
            // POLISH (a stationarity residual above the bar: rounding accumulated over many steps): the point rebuilt from its
            // multipliers, c = c_u + sum u_j C a_j -- stationary up to the table's rounding -- and one refinement of the multipliers that
            // puts the active rows back at zero slack:  rho = h_A - A c,  du = S^-1 rho,  u += du,  c += sum du_j C a_j.  Then every row
            // is looked at again.
#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
            // (this path verifies again: lam_ goes back to zero first -- behind the verification's reduction barrier, so every lane has
            // read it -- where thread 0 added, and only inside lam_: in 2-D an LSC row's third entry names axis 2 with coefficient 0,
            // which addresses plo_ behind lam_, and that word keeps what the sums left in it.  The barriers below publish the zeros.)
            if (tid == 0) {
                for (int j_ = 0; j_ < k; j_++)
#pragma unroll
                    for (int t_ = 0; t_ < 3; t_++) {
                        const int en = aint_[4 * j_ + 1 + t_], at = ent_axis(en) * P + ent_cp(en);
                        if (at < NX) lam_[at] = 0.0;
                    }
            }
#endif
            LSCQP_DAS_BARRIER();
            add_columns(k, u_, cu_);
            LSCQP_DAS_BARRIER();
            if (wv == 0) {
                const double rho = (lane < k) ? arhs_[lane] - row_dot(&aint_[4 * lane + 1], &acoef_[3 * lane], c_) : 0.0;
                const double du = solve_factor(k, rho, nullptr);
                // multipliers >= 0 is the one KKT condition the passes do not look at again: a refined multiplier below zero by more than
                // rounding is not this phase's to return -- the interior-point kernel solves the instance; rounding-size negatives are zero
                const double un = (lane < k) ? u_[lane] + du : 0.0;
                const double umax = DAS_MAX0(fabs(un));
                const double neg = DAS_MAX0((lane < k && un < -1e-12 * umax) ? 1.0 : 0.0);
                if (lane < k) u_[lane] = fmax(un, 0.0);
                if (lane == 0) ctl_[7] = neg;
            }
            LSCQP_DAS_BARRIER();
            if (ctl_[7] != 0.0) {  // (uniform; not solved: handed over below)
                why = LSCQP_DAS_WHY_MULTIPLIER;
                break;
            }
            add_columns(k, r_, nullptr);
            LSCQP_DAS_BARRIER();
            polished = true;
            continue;
        }
        polished = false;
        if constexpr (SCREEN) break;  // (a violated row: the full form's)
        if (k >= kmax) {  // more active rows than this launch holds: the interior-point kernel's
            why = LSCQP_DAS_WHY_ROWS;
            break;
        }
#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
        (void)haveJ, (void)haveC;  // (the prologue has zeroed the factor: nothing to remember)
#else
        if (!haveJ) {  // (before the first step; by wavefront 0, the only one that touches J: in order with its own use)
            if (wv == 0)
                for (int e = lane; e < kcap * LDL; e += 64) Jm_[e] = 0.0;
            haveJ = true;
        }
#endif
        // (kTableEarly: the first pass has left the table in LDS)
        if (!kTableEarly && cacheC && !haveC) {  // the table of this instance's ts in LDS from the first step on (every step reads a few of its columns)
            bool copied = false;
            if constexpr (kCPre > 0) {
                if (c_prefetched) {
#pragma unroll
                    for (int i = 0; i < kCPre; i++) {
                        const int e = tid + i * T;
                        if (e < P * P) Cc_[e] = cpre[i];
                    }
                    copied = true;
                }
            }
            if (!copied)
                for (int e = tid; e < P * P; e += T) Cc_[e] = Cg[e];
            haveC = true;
            Cm = Cc_;
            LSCQP_DAS_BARRIER();  // (every thread reads columns other threads copied)
        }
        // ---- the candidate row p = bid, slot kcap of the descriptors ----
        Row Rp;
        decode(bid, Rp);
        if (tid == 0) {
            aint_[4 * kcap] = bid;
            for (int t = 0; t < 3; t++) aint_[4 * kcap + 1 + t] = Rp.ent[t], acoef_[3 * kcap + t] = Rp.coef[t];
            arhs_[kcap] = Rp.rhs;
            ctl_[3] = 0.0;  // the candidate's multiplier so far
        }
        // w_p = C a_p goes into slot k of W.  Wavefront 0's decision of the first partial step does not read it -- a_p'C a_p comes straight from
        // the table, v_j = a_j'C a_p = a_p'w_j from the columns the active rows already have -- so the OTHER wavefronts compute w_p while
        // wavefront 0 decides, and one barrier serves both (one wavefront per QP: first w_p, then the decision).
        auto compute_wp = [&](int first_thread, int n_threads) {
            for (int e = tid - first_thread; e < NX; e += n_threads) {
                if (e < 0) continue;
                const int kx = fdiv(e, iP), cp = e - kx * P;
                W_[(size_t)k * NX + e] = ccol(Rp.ent, Rp.coef, kx, cp, Cm, P);
            }
        };
        if constexpr (NW == 1) compute_wp(0, T);
        DAS_T(5);  // candidate: decode, table copy (one wavefront: w_p)
        double spp = 0.0;  // a_p'C a_p (wavefront 0)
#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
        // the candidate's multiplier so far, in a register of wavefront 0 beside ctl_[3] (zeroed above, the same sums in the same order:
        // the decision's t is the same in every lane of the wavefront); the decision takes the register instead of a round trip to LDS
        double u_cand = 0.0;
#define DAS_U_CAND u_cand
#else
#define DAS_U_CAND ctl_[3]
#endif
        bool stop = false, first_step = true;
        for (;;) {  // partial steps until p has joined the set
            steps++;
            if (steps > max_steps) {
                stop = true;
                why = LSCQP_DAS_WHY_STEPS;
                break;
            }
            if (NW > 1 && first_step && wv != 0) compute_wp(64, T - 64);
            // Wavefront 0 decides the step: v = A'w_p, r = S^-1 v, curvature a_p'w_p - v'r, dual bound t1, primal length t2.
            if (wv == 0 && __builtin_amdgcn_readfirstlane(k) == 0) {
                // the FIRST active row (most stepping instances of a plan never hold a second): nothing to solve, no row can leave -- the general
                // decision below with k = 0, minus its two reductions and its solve; the same values to the bit
                if (first_step) spp = cdot(Rp.ent, Rp.coef, Rp.ent, Rp.coef, Cm, P);
                const double sp = row_dot(Rp.ent, Rp.coef, c_) - Rp.rhs;
                const double t = (spp > 1e-12 * spp) ? -sp / spp : 1e300;
                const int kind = (t < 1e299) ? 1 : 0;
#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
                u_cand = u_cand + t;
                if (lane == 0) {
                    if (kind == 1) Jm_[0] = rsqrt(spp), u_[0] = u_cand;
                    ctl_[0] = t;
                    ctl_[1] = (double)kind;
                    ctl_[2] = 0.0;
                    ctl_[3] = u_cand;
                    ctl_[5] = (t < 1e299) ? 1.0 : 0.0;
                }
#else
                if (lane == 0) {
                    if (kind == 1) Jm_[0] = rsqrt(spp), u_[0] = ctl_[3] + t;
                    ctl_[0] = t;
                    ctl_[1] = (double)kind;
                    ctl_[2] = 0.0;
                    ctl_[3] += t;
                    ctl_[5] = (t < 1e299) ? 1.0 : 0.0;
                }
#endif
            } else if (wv == 0) {
                if (first_step) spp = cdot(Rp.ent, Rp.coef, Rp.ent, Rp.coef, Cm, P);
                const double vj = (lane < k) ? row_dot(Rp.ent, Rp.coef, W_ + (size_t)lane * NX) : 0.0;
                DAS_T(13);
                double yy;
                const double ri = solve_factor(k, vj, &yy);
                DAS_T(14);
                const double curv = spp - yy;  // a_p'w_p - v'S^-1 v
                const double sp = row_dot(Rp.ent, Rp.coef, c_) - Rp.rhs;
                const double t2 = (curv > 1e-12 * spp) ? -sp / curv : 1e300;
                double t1 = (lane < k && ri > 0.0) ? u_[lane] / ri : 1e300;
                int l = lane;
                DAS_ARGMIN(t1, l);
                const double t = fmin(t1, t2);
                int kind;  // 0: no step exists (hand over); 1: p joins; 2: row l leaves; 3: no step exists and the row is violated beyond what the rest of its normal can repair: no point satisfies the rows
                if (!(t < 1e299)) kind = (sp < -1e-6) ? 3 : 0;  // (3 is a candidate proof: checked after the loop)
                else if (t2 <= t1) kind = 1;
                else kind = 2;
                DAS_T(15);
                if (kind == 1 || kind == 2) {
                    if (lane < k) u_[lane] = fmax(0.0, u_[lane] - t * ri);
                    if (kind == 1) {  // one more row of J: (-r', 1) / sqrt(curv); the column above its diagonal entry is zero
                        const double idl = rsqrt(curv);
                        if (lane < k) Jm_[k * LDL + lane] = -ri * idl, Jm_[lane * LDL + k] = 0.0;
                        if (lane == 0) Jm_[k * LDL + k] = idl, u_[k] = DAS_U_CAND + t;
                    }
                }
#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
                u_cand = u_cand + t;
#endif
                if (lane == 0) {
                    ctl_[0] = t;
                    ctl_[1] = (double)kind;
                    ctl_[2] = (double)l;
#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
                    ctl_[3] = u_cand;
#else
                    ctl_[3] += t;
#endif
                    ctl_[5] = (t2 < 1e299) ? 1.0 : 0.0;  // a primal step is taken
                    ctl_[7] = -sp;
                }
            }
            first_step = false;
            DAS_T(10);  // the step's decision (wavefront 0)
            LSCQP_DAS_BARRIER();
            const double t = ctl_[0];
            const int kind = __builtin_amdgcn_readfirstlane((int)ctl_[1]), l = __builtin_amdgcn_readfirstlane((int)ctl_[2]);  // (uniform: scalar loop bounds)
#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
            // `primal` in the same block of reads as t, kind and l, in front of the test on kind (behind it the read was a round trip of
            // its own; the decision stores ctl_[5] whatever kind it finds)
            double primal_w = ctl_[5];
            asm volatile("" : "+v"(primal_w));
#endif
            if (kind == 0 || kind == 3) {
                stop = true;
                why = LSCQP_DAS_WHY_NO_STEP;
                proven = kind == 3;
                break;
            }
            // c += t (w_p - sum r_j w_j)   (r_ holds this step's r); a leaving row closes the gap in W on the way (the candidate moves down too)
            const int ks = __builtin_amdgcn_readfirstlane(k);  // (uniform by construction; said so: scalar loop bounds)
#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
            const bool primal = __builtin_amdgcn_readfirstlane((int)primal_w) != 0;
#else
            const bool primal = __builtin_amdgcn_readfirstlane((int)ctl_[5]) != 0;
#endif
            for (int e = tid; e < NX; e += T) {
                if (primal) {
                    double a = W_[(size_t)ks * NX + e];
                    for (int j0 = 0; j0 < ks; j0 += 4) {
                        double wj[4], rj[4];
#pragma unroll
                        for (int t_ = 0; t_ < 4; t_++)  // (past the end: the candidate's column with r_'s zero)
                            wj[t_] = W_[(size_t)min(j0 + t_, ks) * NX + e], rj[t_] = r_[j0 + t_];
#pragma unroll
                        for (int t_ = 0; t_ < 4; t_++) a -= rj[t_] * wj[t_];
                    }
                    c_[e] += t * a;
                }
                if (kind == 2) {  // (every thread its own elements: the copies of one element are ordered, those of different elements independent)
                    double nxt = W_[(size_t)(l + 1) * NX + e];
                    for (int j = l; j < ks; j++) {
                        const double cur = nxt;
                        nxt = W_[(size_t)min(j + 2, ks) * NX + e];
                        W_[(size_t)j * NX + e] = cur;
                    }
                }
            }
            DAS_T(11);  // the step itself: c, W
            if (kind == 1) {
#if LSCQP_DAS_FORM == LSCQP_DAS_LATENCY
                // the joining row's descriptors, from the registers every thread holds (slot kcap keeps the copy the candidate left there --
                // nothing has written it since -- and is not read here: eight LDS round trips of one thread in front of the barrier)
                if (tid == 0) {
                    aint_[4 * k] = bid;
#pragma unroll
                    for (int t_ = 0; t_ < 3; t_++) aint_[4 * k + 1 + t_] = Rp.ent[t_], acoef_[3 * k + t_] = Rp.coef[t_];
                    arhs_[k] = Rp.rhs;
                }
#else
                if (tid == 0) {
                    for (int t_ = 0; t_ < 4; t_++) aint_[4 * k + t_] = aint_[4 * kcap + t_];
                    for (int t_ = 0; t_ < 3; t_++) acoef_[3 * k + t_] = acoef_[3 * kcap + t_];
                    arhs_[k] = arhs_[kcap];
                }
#endif
                k++;
                LSCQP_DAS_BARRIER();
                break;
            }
            // row l leaves: close the gap in descriptors and multipliers (lane j takes slot j + 1's: every lane reads before any lane writes),
            // downdate the factor (wavefront 0)
            if (wv == 0) {
                const bool mv = lane >= l && lane + 1 < k;
                const int from = mv ? lane + 1 : 0;
                int ai[4];
                double ac[3];
#pragma unroll
                for (int t_ = 0; t_ < 4; t_++) ai[t_] = aint_[4 * from + t_];
#pragma unroll
                for (int t_ = 0; t_ < 3; t_++) ac[t_] = acoef_[3 * from + t_];
                const double ah = arhs_[from], uu = u_[from];
                LSCQP_DAS_WAVE_SYNC();
                if (mv) {
#pragma unroll
                    for (int t_ = 0; t_ < 4; t_++) aint_[4 * lane + t_] = ai[t_];
#pragma unroll
                    for (int t_ = 0; t_ < 3; t_++) acoef_[3 * lane + t_] = ac[t_];
                    arhs_[lane] = ah, u_[lane] = uu;
                }
            }
            const bool okf = factor_remove(k, l);
            k--;
            if (wv == 0 && lane == 0) ctl_[6] = okf ? 0.0 : 1.0;
            LSCQP_DAS_BARRIER();
            DAS_T(12);  // a leaving row: descriptors, factor
            if (ctl_[6] != 0.0) {
                stop = true;
                why = LSCQP_DAS_WHY_PIVOT;
                break;
            }
        }
        DAS_T(6);  // the partial steps of the candidate
        if (stop) break;
    }
    if (!solved) {
        if (proven) {
            // A proof only if the violation exceeds what the candidate's part outside the active rows' span could still buy: about
            // sqrt(curv / spp) |a_p| per metre travelled, over at most the world box's diameter.  curv = a_p'C a_p - v'r as the last step's
            // decision had it, again from what LDS holds -- the candidate's descriptors (slot kcap), W and r_ -- by every thread alike.
            const int* const pe = &aint_[4 * kcap + 1];
            const double* const pc = &acoef_[3 * kcap];
            double vr = 0.0;
            for (int j = 0; j < k; j++) vr += r_[j] * row_dot(pe, pc, W_ + (size_t)j * NX);
            const double spp = cdot(pe, pc, pe, pc, Cm, P);
            const double d0 = wb_[3] - wb_[0], d1 = wb_[4] - wb_[1], d2 = wb_[5] - wb_[2];
            const double reach = sqrt(fmax(spp - vr, 0.0) / spp * (pc[0] * pc[0] + pc[1] * pc[1] + pc[2] * pc[2]) * (d0 * d0 + d1 * d1 + d2 * d2));
            proven = ctl_[7] > 1e-6 + reach;  // (otherwise: handed over, LSCQP_DAS_WHY_NO_STEP)
        }
        if (proven) infeasible_out(steps, ctl_[7]);
        else hand_over(steps, why);
        DAS_T_FLUSH();
        LSCQP_DAS_END(proven ? kDasInfeasible : kDasHandedOver);
    }

    write_out();
    DAS_T(7);  // epilogue
    DAS_T_FLUSH();
    LSCQP_DAS_END(kDasSolved);
#undef DAS_U_CAND
#undef DAS_CLS
#undef DAS_ARGMIN
#undef DAS_SUM
#undef DAS_MAX0
#undef DAS_MAX0_MAX0_SUM
