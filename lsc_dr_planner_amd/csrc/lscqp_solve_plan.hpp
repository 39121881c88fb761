// lscqp_solve_plan.hpp -- what ONE solve call launches, as data: the launch policy of the dual active-set phase (das_phase_shape) and the chain of
// passes around it (plan_solve).  Host only and pure: nothing here calls HIP, reads the environment, allocates or writes to the handle, so the
// policy is checked on a machine without a device (lscqp_debug_solve_plan_, tests/test_solve_plan_cpu.py).  lscqp_solve_batch_device_internal_
// runs the plan it gets from plan_solve, pass by pass; there is no second copy of any rule.
// Included by lscqp_api.hip alone, behind its Knobs, Inst, fused_fn, find_instance, find_fused and other_order_instance: those stay there with the
// kInst table, and the planner calls them.
#pragma once

namespace {

// Which part of a call is asked for.  The host-pointer entries and lscqp_comm.hip look at the statuses between the parts.
enum SolvePart : int32_t {
    PART_WHOLE = 0,         // everything the call's retry asks for
    PART_BEHIND_PHASE = 1,  // the interior-point passes of a call whose phase has ALREADY run (SolvePlan::deferred)
    PART_OTHER_ORDER = 2,   // only the repair pass on the instance of the other elimination order
    PART_RESCUE = 3,        // only the rescue pass
};
enum PassKind : int32_t { PASS_PRESCREEN = 0, PASS_PHASE = 1, PASS_FUSED = 2, PASS_INSTANCE = 3, PASS_GENERIC = 4 };
enum PlanError : int32_t { PLAN_OK = 0, PLAN_LEAN_WITH_PRESCREEN = 1, PLAN_ONLY_WITHOUT_PHASE = 2, PLAN_NO_KERNEL = 3 };  // all LSCQP_ERR_UNSUPPORTED

// The three structs are also what lscqp_debug_solve_plan_ hands out, field for field (api.py: _Plan): int32 and pointers only.
struct PhaseShape {  // launch shape of the phase (lscqp_launch_das; the fused launcher takes the same budgets)
    int32_t cap;     // obstacles per agent the launch holds
    int32_t threads, kmax, steps, cacheC, stage_rows;
    int32_t screen;  // bit 0 the lean form in front, bit 1 the first look inside the loop of steps, bit 2 skip what the prescreen proved
    int32_t tiny;    // the batch leaves most CUs idle (n <= CUs)
    int32_t lds;     // bytes of LDS per workgroup of this shape
};
struct Pass {
    int32_t kind;          // PassKind
    int32_t repair, scan;  // DevClass::repair, DevClass::scan of the launch
    int32_t queue;         // the launch gets a work-queue counter (next_queue_counter, in launch order)
    int32_t x_init;        // the launch is given the caller's x_init
    int32_t M, dim, es, slots, waves, mixed;  // the kernel instance (slots, waves, mixed: 0 unless compiled)
    const Inst* inst;      // PASS_INSTANCE, PASS_FUSED: its row of kInst
    const char* what;      // "HIP launch failed (<what>): ..."; "" for the plain text of the first pass
};
constexpr int kPlanPasses = 6;  // prescreen, fused, phase, first pass, second pass, rescue
struct SolvePlan {
    int32_t n_pass;
    int32_t deferred;  // the call returns behind the phase; the caller enqueues PART_BEHIND_PHASE if the phase left an instance
    int32_t error;     // PlanError; nothing is launched
    int32_t capacity;  // kPlanPasses
    PhaseShape phase;  // of the PASS_PHASE / PASS_FUSED, if any
    fused_fn fused;
    // A PASS_FUSED is followed by the PASS_PHASE and the first PASS_INSTANCE it replaces: the executor skips those two when the fused launcher
    // accepts, and runs them when it refuses the budgets for its compiled carve (hipErrorNotSupported) -- the one decision left to run time.
    Pass pass[kPlanPasses];
};

// Does this part of a call try the phase (and so need the class's tables on the device)?
inline bool phase_asked(const lscqp_class_desc& d, const Knobs& kn, SolvePart part) {
    const bool off = kn.active_set_off && d.active_set != LSCQP_ACTIVE_SET_ONLY;
    return part == PART_WHOLE && d.active_set != LSCQP_ACTIVE_SET_OFF && !off;
}

// ---- the launch policy of the DUAL ACTIVE SET phase (lscqp_das.hip) ---------------------------------------------------------------------
// A batch that leaves the chip idle gets four wavefronts per QP, the whole budget of active rows and the class's table in LDS (latency); a
// batch that fills it gets one wavefront per QP and a small LDS footprint (occupancy is what hides the row reads), and the few instances
// with more active rows than that fall to the interior-point kernel.  cap and bit 2 of screen are the planner's.
inline PhaseShape das_phase_shape(const Knobs& kn, int M, int dim, int64_t n, int n_obs_max, int n_cu) {
    // Launch shape (measured, profiles/r05_das_launch_shapes.txt): up to two QPs per CU the launch is about latency -- four
    // wavefronts per QP, the whole budget of active rows, the class's table and the instance's rows in LDS; up to eight per CU
    // the launch still lasts as long as its slowest QP (1024 x M10 x 40: 0.28 ms with one wavefront per QP, 0.19 ms with four) but
    // LDS is what limits the resident workgroups -- four wavefronts, a small footprint; beyond that one wavefront per QP.
    const int64_t ncu = n_cu > 0 ? n_cu : 256;
    const bool small = n <= 2 * ncu, medium = n <= 8 * ncu;
    auto knob = [](int v, int dflt) { return v >= 0 ? v : dflt; };  // (overrides: lscqp_debug_set_knob_, tests and sweeps only)
    PhaseShape s{};
    s.threads = knob(kn.das_threads, medium ? 256 : 64);
    // (20 active rows, not the 32 the kernel could hold: the footprint decides how many workgroups a CU holds at once and whether the
    // instance's rows fit in LDS beside the rest -- 512 x M6: 43.0 -> 33.9 us, 128 x M10 x 40: 92.2 -> 84.3, 64 x M5: 12.9 -> 12.5; 24 would
    // already cost the M = 10 class its staged rows.  No feasible instance of a 6 000-instance sweep of the harder swarms needs more than
    // 12; ONE of the ~50 000 of the stress sweep needs 17-20, and at 16 it went to the interior-point kernel, which accepted it at its
    // rounding floor (stationarity 1.9e-7): profiles/r05_kmax_sweep.txt, NOTES.md section 13)
    // round 6 (tools/loaded_probe.py, swarms 8 - 30 replans into their exchange): a batch that leaves most CUs idle (n <= CUs) gets every
    // active row the kernel can hold -- the forest10 class mid-exchange holds > 20 rows at one agent's optimum for several replans, and
    // handing that ONE instance over cost the call 0.16 ms of phase + 0.34 ms of interior point against 0.34 ms without the phase; the
    // step budget of the other small batches is halved: a feasible instance of the loaded sweeps needs <= 50 steps (<= 33 beyond 64 agents),
    // an instance that keeps adding and dropping beyond that is, on those sweeps, one whose rows admit no point -- the kernel behind
    // says so in 14 iterations, and every step spent here before that is added to the call
    const bool tiny = s.tiny = n <= ncu;
    int kmax = knob(kn.das_kmax, tiny ? 32 : small ? 20 : 8);
    s.steps = knob(kn.das_steps, tiny ? 96 : small ? 48 : 24);
    int cacheC = knob(kn.das_cache, small ? 1 : 0);
    int stage = knob(kn.das_stage, small ? 1 : 0) ? n_obs_max * 6 * M : 0;
    // form: bit 0 the lean form in front (built and measured, no gain: the phase is bound by instruction issue, not occupancy); bit 1 the
    // first look inside the loop of steps (one copy of that code: batches of at most two workgroups per CU; lscqp_das.hip, PEEL)
    s.screen = (knob(kn.das_screen, 0) ? 1 : 0) | (knob(kn.das_loop, small ? 1 : 0) ? 2 : 0);
    auto over = [&](int k, int c, int st) { return lscqp_das_lds_bytes(M, dim, k, c, st) > lscqp::kMaxLdsBytes; };
    // what does not fit the CU's LDS is given up in this order: staged rows, the table copy, active rows.
    // (For the shapes the library accepts, M <= 12, giving up the staged rows always suffices: without them the footprint is at most
    // 130 704 B -- M = 12, dim 3, 32 rows, with the table copy -- against the 163 840 B of a CU.  Every `cacheC = 0` below and the loop over
    // kmax are therefore UNREACHABLE for every budget the kernel holds, kmax <= 32.  Kept as they were.)
    if (over(kmax, cacheC, stage)) stage = 0;
    if (over(kmax, cacheC, stage)) cacheC = 0;
    // THE RETREAT QUIRK: the test below asks whether 32 rows fit WITH the staged rows and the table copy -- also when the staged rows were
    // just given up above and 32 rows would fit without them.  n <= CUs, M = 10, dim 3, 64 obstacles: the staged rows go (they do not fit
    // beside 20 rows either), and the batch is cut to 20 rows at 81 392 B although 32 fit with room to spare.  Pinned by
    // tests/test_solve_plan_cpu.py; whoever tunes the policy next decides whether it stays.
    if (tiny && kn.das_kmax < 0 && kmax > 20 && over(kmax, knob(kn.das_cache, 1), knob(kn.das_stage, 1) ? n_obs_max * 6 * M : 0)) {
        // (the larger budget never at the price of the staged rows or the table copy: 128 x M10 x 40 runs 8 % slower without them)
        kmax = 20;
        cacheC = knob(kn.das_cache, 1);
        stage = knob(kn.das_stage, 1) ? n_obs_max * 6 * M : 0;
        if (over(kmax, cacheC, stage)) stage = 0;
        if (over(kmax, cacheC, stage)) cacheC = 0;
    }
    while (kmax > 4 && over(kmax, cacheC, stage)) kmax -= 4;
    s.kmax = kmax, s.cacheC = cacheC, s.stage_rows = stage;
    s.lds = (int32_t)lscqp_das_lds_bytes(M, dim, kmax, cacheC, stage);
    return s;
}

// ---- the plan of one call ------------------------------------------------------------------------------------------------------------
// n_cu is the device's CU count as cu_count() reports it (0: unknown -- every batch then counts as one that fills the chip, except for the
// phase's shape, which assumes 256); tables: the class's active-set tables are on the device (das_device_table); deferred: the caller looks at
// the statuses behind the phase before it asks for PART_BEHIND_PHASE.  retry is 0 .. 3 and is not read for the two single-pass parts.
inline SolvePlan plan_solve(const lscqp_class_desc& d, int es, const Knobs& kn, int prescreen, int64_t n, int n_obs_max, int retry, SolvePart part,
                            bool has_x_init, bool deferred, int n_cu, bool tables) {
    SolvePlan p{};
    p.capacity = kPlanPasses;
    const int M = d.M, dim = d.dim;
    auto add = [&](PassKind kind, const Inst* i, int repair, int scan, bool queue, bool x_init, const char* what) {
        if (p.n_pass < kPlanPasses)
            p.pass[p.n_pass++] = Pass{kind, repair, scan, queue, x_init, M, dim, es, i ? slots_of(*i) : 0, i ? i->waves : 0, i ? i->mixed : 0, i, what};
    };
    const int mixed = d.precision == LSCQP_PRECISION_MIXED ? 1 : 0;
    const bool only = d.active_set == LSCQP_ACTIVE_SET_ONLY;
    const bool single = part == PART_OTHER_ORDER || part == PART_RESCUE;
    if (single && only) return p;  // (the host-pointer entries' extra passes are interior-point passes)
    const Inst* inst = find_instance(kn, M, dim, es, mixed, n_obs_max, n, n_cu);
    const Inst* inst64 = mixed ? find_instance(kn, M, dim, es, 0, n_obs_max, n, n_cu) : inst;
    const bool compiled = inst && inst64;
    // (asked only where a rule needs it -- never on the compiled chain of a call without a rescue pass: a 12 us call counts its host work)
    auto generic_holds = [&] { return n_obs_max <= lscqp_generic_max_obstacles(M, dim, es); };
    const bool no_kernel = !compiled && (mixed || !generic_holds());
    // a launch of more instances than the device has CUs MAY exceed what the chip holds at once: it gets a zeroed work-queue counter and
    // the instance's launcher decides (lscqp_inst.hip: persistent workgroups over the queue, or one instance per workgroup)
    // (a counter -- a memset on the stream, a slot of the ring -- only for a launch that can use it: the instance has a persistent form, and
    // the pass is not the near-empty one behind the dual active-set phase, where almost every workgroup returns at once)
    const bool queued = !kn.no_queue && n > (int64_t)n_cu;  // (no_queue: tools/lpt_probe.py tells the queue and the order apart)
    // ---- the PRESCREEN (lscqp_prescreen.hip), in front of everything: what it proves infeasible is final (LSCQP_INFO_ACTIVE_SET |
    // LSCQP_INFO_PRESCREENED), everything else is marked ITER_LIMIT -- the phase skips the former through bit 2 of its form, and a first
    // interior-point pass without the phase in front runs the way the pass behind the phase does (repair = 3: only what is marked)
    const bool prescreened = prescreen == LSCQP_PRESCREEN_ON && !single;
    if (prescreened && kn.das_screen > 0) {
        p.error = PLAN_LEAN_WITH_PRESCREEN;
        return p;
    }
    if (prescreened && part == PART_WHOLE) add(PASS_PRESCREEN, nullptr, 0, 0, false, has_x_init, "prescreen");
    // ---- the PHASE in front of the first interior-point pass: one launch over the batch; what it finishes is OPTIMAL
    // (LSCQP_INFO_ACTIVE_SET), everything else is marked for the interior-point kernel, whose first pass then runs with repair = 3 (skip
    // what is OPTIMAL, nothing was "repaired")
    bool das_ran = part == PART_BEHIND_PHASE;
    if (phase_asked(d, kn, part)) {
        const int cap = compiled ? std::min(inst->max_obs, inst64->max_obs) : (no_kernel ? -1 : n_obs_max);
        const PhaseShape s = (tables && cap >= 0) ? das_phase_shape(kn, M, dim, n, n_obs_max, n_cu) : PhaseShape{};
        if (tables && cap >= 0 && (size_t)s.lds <= lscqp::kMaxLdsBytes) {
            p.phase = s;
            p.phase.cap = cap;
            p.phase.screen |= prescreened ? 4 : 0;  // (lscqp_launch_das: the phase skips what the prescreen marked INFEASIBLE)
            // FUSED (lscqp_fused.hip): a batch of at most one instance per CU whose phase runs in its small-batch form on fp64 rows, in front of
            // an fp64 instance that has a fused form, gets ONE launch -- a workgroup that hands its instance over solves it itself, with the
            // pass's own class (repair = 3).  The separate pass behind the phase was a launch of n workgroups that almost all load a status and
            // leave: 64 x M5, 14.25 -> 11.82 us per call fused (profiles/r07_fused.txt).  Not for calls that look at the statuses before they
            // enqueue the pass (`deferred`), nor behind the scan form.
            if (kn.das_fused && !prescreened && s.tiny && !mixed && !kn.behind_scan && !only && !deferred && s.threads == 256 && s.screen == 2 &&
                d.row_format != LSCQP_ROWS_F32)
                p.fused = find_fused(inst);
            if (p.fused) add(PASS_FUSED, inst, 3, 0, false, has_x_init, "fused active-set phase");
            add(PASS_PHASE, nullptr, 0, 0, false, has_x_init, "dual active-set phase");
            das_ran = true;
        }
        if (only) {
            if (!das_ran) p.error = PLAN_ONLY_WITHOUT_PHASE;
            return p;
        }
        if (das_ran && deferred) {  // the caller looks at the statuses first
            p.deferred = 1;
            return p;
        }
    }
    if (no_kernel) {
        p.error = PLAN_NO_KERNEL;
        return p;
    }
    const int first_repair = (das_ran || prescreened) ? 3 : 0;
    // RESCUE pass (PART_RESCUE: only it; retry 2 and 3: after the other passes): what is still at the iteration limit or broke down numerically
    // goes through the run-time-shaped kernel once more with repair = 2 (lscqp_generic.hip: weighted corrector), never with a queue counter
    auto add_rescue = [&] { add(PASS_GENERIC, nullptr, 2, 0, false, false, "rescue pass"); };
    if (!compiled) {
        // no compiled instance serves this launch (shape without one, or more obstacles than its register slots hold): the
        // run-time-shaped kernel, fp64.  Same statuses, same second pass; no other elimination order to try.
        if (part == PART_RESCUE) add_rescue();
        if (single) return p;
        add(PASS_GENERIC, nullptr, first_repair, 0, false, has_x_init, "run-time-shaped kernel");
        if (retry && has_x_init) add(PASS_GENERIC, nullptr, 1, 0, false, false, "run-time-shaped kernel, second pass");
        if (retry == 2 || retry == 3) add_rescue();
        return p;
    }
    if (part == PART_RESCUE) {
        if (generic_holds()) add_rescue();  // (else the kernel cannot hold the batch: nothing to try)
        return p;
    }
    if (part == PART_OTHER_ORDER) {  // the statuses of a first pass are in d_status_out
        const Inst* other = other_order_instance(inst64, n_obs_max);
        if (other) add(PASS_INSTANCE, other, 1, 0, queued && other->persist, false, "other-order pass");
        return p;
    }
    // Behind the phase the pass usually finds nothing to do, and what it costs then is its launch: n workgroups that load one status each and
    // leave (4096 x M5: 4.5 us and 33 MB of fetches per call; a mixed-precision class: two such launches, float32 then fp64).  So behind the
    // phase the pass runs on an fp64 instance of the same capacity that has the PERSIST form, in its scan mode (lscqp_kernel.hpp:
    // DevClass::scan): at most as many workgroups as the chip holds, each looking through 64 statuses per round trip.  A mixed-precision class
    // is served by that fp64 instance directly -- the float32 factorisation has nothing to add behind a phase that finishes the easy
    // instances, and its own second pass would be a third launch.  Without such an instance: as before.
    const bool scan_form = das_ran && kn.behind_scan;
    const Inst* first = inst;
    int first_scan = 0;
    if (das_ran && !scan_form) {
        // MEASURED (round 6, profiles/r06_behind_scan.txt): the scan form LOSES -- 64 x M5 14.8 -> 17.3 us per call, 4096 x M5 41.0 -> 42.3 -- the
        // persistent form of the kernel pays more before its first status load than n one-status workgroups cost.  Off by default (knob
        // behind_scan); what stays is the mixed-precision class going straight to its fp64 instance behind the phase (one launch instead of two).
        first = mixed ? inst64 : inst;
    } else if (scan_form) {
        const int want = std::min(inst->max_obs, inst64->max_obs);
        if (!(inst->persist && !inst->mixed)) {
            const Inst* b = nullptr;
            for (const Inst& i : kInst)
                if (i.M == M && i.dim == dim && i.es == es && !i.mixed && i.persist && i.max_obs == want && (!kn.pin_waves || i.waves == kn.pin_waves) &&
                    (!b || i.waves < b->waves))
                    b = &i;
            first = b ? b : (mixed ? inst64 : inst);
        }
        first_scan = (first->persist && !first->mixed) ? 1 : 0;
    }
    add(PASS_INSTANCE, first, first_repair, first_scan, queued && first->persist && !das_ran, has_x_init, "");
    // Second pass over the batch, same stream, no host round trip: a workgroup whose instance is already OPTIMAL (or was
    // refused for capacity) returns at once.  Mixed precision: the fp64 kernel re-solves what the float32 factorisation could
    // not finish (same start).  retry: the fp64 kernel re-solves from the DEFAULT start what a warm start did not bring to
    // OPTIMAL -- a jammed or diverged warm start (ITER_LIMIT / NUMERIC, or relabelled INFEASIBLE on its primal residual) says
    // nothing about the problem, a cold start proves infeasibility independently of x_init.
    // retry = 2: the second pass on the instance of the other elimination order (also for cold batches).  Not the default of a retry:
    // the natural-order instances of the shapes that have both spill to scratch, and a kernel with a private segment costs ~35 us to
    // launch even when every workgroup returns at once (measured: 38.7 vs 4.6 us per call on the forest10 replica).
    const Inst* alt = retry == 2 ? other_order_instance(inst64, n_obs_max) : nullptr;
    if ((mixed && first->mixed) || (retry && (has_x_init || alt))) {
        // (behind the phase the second pass, too, finds nothing on most batches: same instance, same scan form as the first)
        const Inst* second = alt ? alt : ((scan_form && first->persist && !first->mixed) ? first : inst64);
        const int scan = (scan_form && second->persist) ? 1 : 0;
        add(PASS_INSTANCE, second, 1, scan, queued && !scan && second->persist, !retry && has_x_init, "second pass");
    }
    if ((retry == 2 || retry == 3) && generic_holds()) add_rescue();
    return p;
}

}  // namespace
