"""Development aid: are two builds of the library the SAME code path?  (profiles/r18_solve_plan.txt, NOTES.md section 26)
  python tools/solve_plan_ab.py libA.so libB.so     every case below on each library, in a fresh process each; a hash of (x, obj, status,
                                                    info) per case; the two lists must be identical
  python tools/solve_plan_ab.py --child OUT         (LSCQP_LIB names the library) the cases, one "name hash" line each into OUT -- also the
                                                    program to put behind `rocprofv3 --kernel-trace -d DIR --`
  python tools/solve_plan_ab.py --traces DIRA DIRB  the ordered (kernel, grid, workgroup, LDS) lists of two such traces must be identical
Cases, around each of the batches c1, c1_loaded, c1_infeasible_1pct, c0_loaded, c3s of bench.CONFIGS, one factor at a time: retry 0..3 with and
without x_init; n cut or repeated to 1, 64, CUs, CUs + 1, 2 CUs + 1, 8 CUs + 1; the prescreen; active_set OFF / ONLY; mixed precision; the knobs
force_generic, pin_waves, behind_scan, no_queue, das_fused (at the batch's size and at 2 CUs + 1); the host-pointer entry with defer_behind 0
and 1, two calls each; one sharded call on a one-device communicator."""
import csv
import glob
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = ("c1", "c1_loaded", "c1_infeasible_1pct", "c0_loaded", "c3s")


def child(out_path):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import bench
    from lsc_dr_planner_amd import api, synth

    dev = torch.device("cuda", 0)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    lines = []

    def digest(*arrays):
        h = hashlib.sha256()
        for a in arrays:
            h.update(np.ascontiguousarray(a).view(np.uint8).tobytes())
        return h.hexdigest()[:24]

    def resized(arrays, x0, n0, n):  # the first n instances of the batch repeated
        hdr, rows, off, sfc = arrays[0], arrays[1].reshape(-1), arrays[2], arrays[3]
        reps = -(-n // n0)
        offs = np.concatenate([off[:-1] + r * off[-1] for r in range(reps)] + [[reps * off[-1]]]).astype(np.uint64)[:n + 1]
        per = len(sfc) // n0
        return (np.concatenate([hdr] * reps)[:n], np.concatenate([rows] * reps)[:int(offs[-1])], offs, np.concatenate([sfc] * reps)[:n * per]), \
            np.concatenate([x0] * reps)[:n]

    for key in BATCHES:
        cfg = bench.CONFIGS[key]
        N, M, dim = cfg["agents"], cfg["segments"], cfg["dim"]
        sw, _, build, arrays0 = bench.make_batch(api, synth, lambda s: api.Solver(api.make_desc(M=M, dim=dim, world_min=s.world_min, world_max=s.world_max)),
                                                 N, M, dim, cfg["obs"], seed=cfg["seed"], style=cfg["style"], warm_steps=cfg.get("warm_steps", 3))
        arrays0 = list(arrays0)
        if cfg.get("infeasible_frac"):
            arrays0[1], _ = bench.make_infeasible(api, arrays0[1], arrays0[0], sw.n_obs, M, cfg["infeasible_frac"], cfg["seed"] + 17)
        x00 = np.ascontiguousarray(api.x_init_from_swarm(build, dim), dtype=np.float64).reshape(N, -1)
        n_obs = sw.n_obs
        base = dict(M=M, dim=dim, world_min=sw.world_min, world_max=sw.world_max)
        has_mixed = (M, dim) in ((5, 3), (10, 2))

        def device_case(name, n=N, retry=1, x_init=True, knobs=(), prescreen=False, **desc):
            arrays, x0 = resized(arrays0, x00, N, n)
            sol = api.Solver(api.make_desc(**base, **desc))
            for k, v in knobs:
                sol.set_knob(k, v)
            if prescreen:
                sol.set_prescreen(api.PRESCREEN_ON)
            t = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev) for a in arrays]
            d_xi = torch.from_numpy(x0.reshape(-1).copy()).to(dev) if x_init else None
            d_x = torch.zeros(n * sol.nv, dtype=torch.float64, device=dev)
            d_obj = torch.zeros(n, dtype=torch.float64, device=dev)
            d_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
            d_info = torch.zeros(n * api.INFO_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            try:
                sol.solve_device(n, n_obs, *t, d_x, d_obj, d_st, d_info, d_x_init=d_xi, retry=retry)
                torch.cuda.synchronize()
                h = digest(d_x.cpu().numpy(), d_obj.cpu().numpy(), d_st.cpu().numpy(), d_info.cpu().numpy())
            except api.LscqpError as ex:
                h = "ERROR %s" % ex
            lines.append("%s/%s %s" % (key, name, h))
            sol.close()

        for retry in range(4):
            for xi in (True, False):
                device_case("retry%d_%s" % (retry, "warm" if xi else "cold"), retry=retry, x_init=xi)
        for n in (1, 64, ncu, ncu + 1, 2 * ncu + 1, 8 * ncu + 1):
            device_case("n%d" % n, n=n)
            device_case("n%d_prescreen" % n, n=n, prescreen=True)
        for name, aset in (("off", api.ACTIVE_SET_OFF), ("only", api.ACTIVE_SET_ONLY)):
            device_case("active_set_" + name, active_set=aset)
            device_case("active_set_%s_n%d" % (name, 2 * ncu + 1), n=2 * ncu + 1, active_set=aset)
        if has_mixed:
            for n in (N, 2 * ncu + 1):
                device_case("mixed_n%d" % n, n=n, precision=api.PRECISION_MIXED)
                device_case("mixed_n%d_phase_off" % n, n=n, precision=api.PRECISION_MIXED, knobs=(("active_set_off", 1),))
                device_case("mixed_n%d_behind_scan" % n, n=n, precision=api.PRECISION_MIXED, knobs=(("behind_scan", 1),))
        for knob, v in (("force_generic", 1), ("pin_waves", 1), ("pin_waves", 2), ("pin_waves", 4), ("behind_scan", 1), ("no_queue", 1), ("das_fused", 0)):
            for n in (N, 2 * ncu + 1):
                device_case("%s%d_n%d" % (knob, v, n), n=n, retry=3, knobs=((knob, v),))
                device_case("%s%d_n%d_phase_off" % (knob, v, n), n=n, retry=2, knobs=((knob, v), ("active_set_off", 1)))
        # the host-pointer entry: two consecutive calls per handle, so that its memory of the last call's phase (behind_needed) is exercised
        for defer in (0, 1):
            for tag, knobs in (("", ()), ("_handover", (("das_kmax", 1), ("das_steps", 1)))):  # (handover: the phase leaves most instances)
                sol = api.Solver(api.make_desc(**base))
                sol.set_knob("defer_behind", defer)
                for k, v in knobs:
                    sol.set_knob(k, v)
                for call in range(2):
                    r = sol.solve_host(*arrays0, x_init=x00)
                    lines.append("%s/host_defer%d%s_call%d %s" % (key, defer, tag, call, digest(r["x"], r["obj"], r["status"], r["info"])))
                sol.close()
        try:
            comm = api.Comm(n_devices=1)
            sol = api.Solver(api.make_desc(**base))
            comm.prepare(sol)
            r = sol.solve_sharded(comm, *arrays0, x_init=x00)
            lines.append("%s/sharded %s" % (key, digest(r["x"], r["obj"], r["status"], r["info"])))
            sol.close()
            comm.close()
        except Exception as ex:  # noqa: BLE001  (a machine that does not allow a communicator: recorded, the same on both sides)
            lines.append("%s/sharded UNAVAILABLE %s" % (key, type(ex).__name__))
        print("%s: %d cases so far" % (key, len(lines)), flush=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("%d cases -> %s" % (len(lines), out_path))


def launches(trace_dir):
    paths = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(paths) == 1, (trace_dir, paths)
    rows = list(csv.DictReader(open(paths[0])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    cols = ("Kernel_Name", "Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z", "Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z", "LDS_Block_Size")
    return [tuple(r[c] for c in cols) for r in rows]


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2])
    if sys.argv[1] == "--traces":
        # (the HIP runtime's own copy and fill kernels are left out: how many chunks a host-to-device copy of pageable memory takes is the
        # runtime's timing, not the program's)
        a, b = ([r for r in launches(d) if not r[0].startswith("__amd_rocclr_")] for d in sys.argv[2:4])
        ours = [r for r in a if "lscqp" in r[0]]
        print("%d / %d launches (%d of the library's kernels, %d distinct)" % (len(a), len(b), len(ours), len(set(r[0] for r in ours))))
        bad = [(k, x, y) for k, (x, y) in enumerate(zip(a, b)) if x != y]
        print("IDENTICAL launch lists" if len(a) == len(b) and not bad else "DIFFERENT: first %s" % (bad[:3],))
        return 0 if len(a) == len(b) and not bad else 1
    outs = []
    for lib in sys.argv[1:3]:
        out = os.path.join(os.environ.get("AB_OUT", "."), "solve_plan_ab_%s.txt" % os.path.basename(lib).replace(".so", ""))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], env=dict(os.environ, LSCQP_LIB=os.path.abspath(lib)))
        if r.returncode != 0:
            print("child failed on %s: exit %d" % (lib, r.returncode))
            return 2
        outs.append(open(out).read().splitlines())
    diff = [(x, y) for x, y in zip(*outs) if x != y]
    errors = [x for x in outs[0] if "ERROR" in x]
    print("%d / %d cases, %d differ, %d are error returns" % (len(outs[0]), len(outs[1]), len(diff), len(errors)))
    for d in diff[:20]:
        print("DIFF", d)
    print("IDENTICAL" if len(outs[0]) == len(outs[1]) and not diff else "DIFFERENT")
    return 0 if len(outs[0]) == len(outs[1]) and not diff else 1


if __name__ == "__main__":
    sys.exit(main())
