"""Timing of the prescreen (include/lscqp.h): the solve call with the prescreen off and on, and the prescreen kernel alone against the bytes
it reads, on four batches -- 64 x M5 x 20 and 4096 x M5 x 20, quiet and with bench.make_infeasible's instances (1 of 64; 1 %).
usage: python tools/prescreen_timing.py lib.so [parent_lib.so]
Each (library, batch) pair runs in its own process, HIP events around 200 calls, five interleaved repeats; a library that predates the
prescreen (the parent commit's build) is measured with the prescreen off only -- "off costs nothing" is then read against the parent's own
run-to-run spread.  Prints one line per (batch, library) and, with PRESCREEN_TIMING_OUT set, writes the table there."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = [("64 x M5 x 20, quiet", "c1", 0.0), ("64 x M5 x 20, 1 of 64 infeasible", "c1", 1 / 64),
           ("4096 x M5 x 20, quiet", "c4_f64", 0.0), ("4096 x M5 x 20, 1 % infeasible", "c4_f64", 0.01)]
CHILD = r'''
import os, sys, json
sys.path.insert(0, %r)
import numpy as np, torch
import bench
from lsc_dr_planner_amd import api, synth
key, frac = sys.argv[1], float(sys.argv[2])
cfg = bench.CONFIGS[key]
N, M, dim = cfg["agents"], cfg["segments"], cfg["dim"]
sw, sol, build, (hdr, rows, off, sfc) = bench.make_batch(api, synth, lambda s: api.Solver(api.make_desc(M=M, dim=dim, world_min=s.world_min, world_max=s.world_max)),
                                                         N, M, dim, cfg["obs"], seed=cfg["seed"], style=cfg["style"], warm_steps=3)
if frac > 0:
    rows, bad = bench.make_infeasible(api, rows, hdr, sw.n_obs, M, frac, cfg["seed"] + 1)
dev = torch.device("cuda", 0)
t = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev) for a in (hdr, rows, off, sfc)]
d_xi = torch.from_numpy(np.ascontiguousarray(api.x_init_from_swarm(build, dim))).to(dev)
d_x = torch.zeros(N * sol.nv, dtype=torch.float64, device=dev); d_obj = torch.zeros(N, dtype=torch.float64, device=dev)
d_st = torch.full((N,), -1, dtype=torch.int32, device=dev); d_info = torch.zeros(N * 32, dtype=torch.uint8, device=dev)
has = hasattr(api.lib(), "lscqp_set_prescreen")
def timed(fn, calls=200):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3  # us per call
solve = lambda: sol.solve_device(N, sw.n_obs, t[0], t[1], t[2], t[3], d_x, d_obj, d_st, d_info, d_x_init=d_xi)
out = {"off_us": round(timed(solve), 2)}
st = d_st.cpu().numpy()
out["off_status"] = np.bincount(st, minlength=5).tolist()
if has:
    sol.set_prescreen(api.PRESCREEN_ON)
    out["on_us"] = round(timed(solve), 2)
    st = d_st.cpu().numpy(); fl = d_info.cpu().numpy().view(api.INFO_DTYPE)["flags"]
    out["on_status"] = np.bincount(st, minlength=5).tolist()
    out["prescreened"] = int(((fl & api.INFO_PRESCREENED) != 0).sum())
    sol.set_prescreen(api.PRESCREEN_OFF)
    d_cert = torch.zeros(N * 72, dtype=torch.uint8, device=dev)
    out["alone_us"] = round(timed(lambda: sol.prescreen_device(N, sw.n_obs, t[0], t[1], t[2], t[3], d_cert)), 2)
    nbytes = t[0].numel() + t[1].numel() + t[2].numel() + t[3].numel() + d_cert.numel()  # every row read once, headers, boxes, certificates
    out["alone_bytes"] = int(nbytes)
    out["alone_GBps"] = round(nbytes / (out["alone_us"] * 1e-6) / 1e9, 1)
print(json.dumps(out))
''' % ROOT


def main():
    libs = sys.argv[1:]
    if not libs:
        sys.exit(__doc__)
    rounds = int(os.environ.get("PRESCREEN_TIMING_ROUNDS", "5"))
    lines = []
    for name, key, frac in BATCHES:
        res = {l: [] for l in libs}
        for _ in range(rounds):
            for l in libs:  # interleaved
                o = subprocess.run([sys.executable, "-c", CHILD, key, repr(frac)], env=dict(os.environ, LSCQP_LIB=os.path.abspath(l)), capture_output=True,
                                   text=True, timeout=600)
                line = [x for x in o.stdout.splitlines() if x.startswith("{")]
                res[l].append(json.loads(line[-1]) if line else {"error": o.stderr[-300:]})
        for l in libs:
            lines.append("%-36s %-24s %s" % (name, os.path.basename(l), json.dumps(res[l])))
            print(lines[-1], flush=True)
    if os.environ.get("PRESCREEN_TIMING_OUT"):
        with open(os.environ["PRESCREEN_TIMING_OUT"], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
