"""Build liblscqp.so (the C-ABI library of include/lscqp.h) for gfx950 with hipcc, in-tree.

One translation unit per kernel instance, compiled in parallel; hipcc cross-compiles without a GPU.
"""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
_AB = os.environ.get("LSCQP_AB", "")  # development: LSCQP_AB=<name> builds liblscqp_<name>.so from its own object directory
OBJ = os.path.join(HERE, "csrc", "_obj" + ("_" + _AB if _AB else ""))
LIB = os.path.join(HERE, "liblscqp%s.so" % ("_" + _AB if _AB else ""))
SYNC_LIB = os.path.join(HERE, "liblscqp%s_sync.so" % ("_" + _AB if _AB else ""))  # the race test's twin (csrc/lscqp_das.hip: LSCQP_DAS_FULL_SYNC)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# -disable-promote-alloca-to-vector: the kernel keeps its per-lane row state in small arrays indexed by fully unrolled
# loops.  AMDGPUPromoteAlloca turns them into 512/1024-bit vector registers BEFORE the loops are unrolled and SROA could
# split them into scalars; every single-element access then moves a whole 16/32-register tuple between AGPRs and VGPRs
# (measured on MI355X: 0.192 -> 0.158 ms per 64-QP batch, 0.875 -> 0.671 ms per 4096-QP batch, scratch 336 -> 0 B/lane).
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-mllvm", "-disable-promote-alloca-to-vector",
         "-Wall", "-Wno-unused-variable", "-Wno-unused-but-set-variable"] + os.environ.get("LSCQP_EXTRA_FLAGS", "").split()


def instances():
    txt = open(os.path.join(CSRC, "lscqp_launch.hpp")).read()
    body = txt[txt.index("#define LSCQP_INSTANCES"):]
    return [tuple(int(v) for v in m) for m in re.findall(r"X\((\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+)\)", body)]


def fused_instances():
    txt = open(os.path.join(CSRC, "lscqp_launch.hpp")).read()
    body = txt[txt.index("#define LSCQP_FUSED_INSTANCES"):]
    body = body[:body.index("\n")]
    return [tuple(int(v) for v in m) for m in re.findall(r"X\((\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+)\)", body)]


def fused_flags(M, D):
    """Optimiser options of one fused unit.  The units that compile the phase's latency text (csrc/lscqp_fused.hip: LSCQP_DAS_FORM -- M = 5,
    and M = 10 in 2-D) are built without machine-level loop-invariant code motion: in front of the loop of steps it hoists the set-up of
    arms the stepping instance of a small batch never enters (the polish, a leaving row, the hand-over, the proof), and what it hoists it
    spills -- without it those units spill 150 / 196 scalar registers against 161 / 220 and the stepping instance is faster in the timing
    twin (NOTES.md section 45).  The throughput unit keeps the default: its machine code is unchanged."""
    return ["-mllvm", "-disable-machine-licm"] if M == 5 or (M == 10 and D == 2) else []


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("command failed: %s\n%s\n%s" % (" ".join(cmd), r.stdout, r.stderr))
    return r.stderr


def _workers(jobs):
    # (a GPU machine shows hundreds of CPUs and allows a command 16)
    return jobs or int(os.environ.get("MAX_JOBS") or 0) or min(os.cpu_count() or 4, 16)


def _env(name):
    return os.environ.get(name, "").split() if name else []


def units():
    """Every translation unit: (source, object name, extra flags, LSCQP_EXTRA_* variable or None, has a _sync twin), in link order."""
    rows = []
    for (M, D, E, S, W, X) in instances():
        rows.append(("lscqp_inst.hip", "inst_%d_%d_%d_%d_%d_%d" % (M, D, E, S, W, X),
                     ["-DLSCQP_M=%d" % M, "-DLSCQP_DIM=%d" % D, "-DLSCQP_ES=%d" % E, "-DLSCQP_NSLOT=%d" % S, "-DLSCQP_W=%d" % W, "-DLSCQP_MIXED=%d" % X],
                     "LSCQP_EXTRA_MIXED_FLAGS" if X else "LSCQP_EXTRA_F64_FLAGS", False))
    # the fused forms (csrc/lscqp_fused.hip): phase + first interior-point pass in one launch; built like the instances (the phase's half keeps
    # its own fp contraction through lscqp_das.hpp's pragma), and a second time from the race test's twin of the phase for liblscqp_sync.so
    for (M, D, E, S, W) in fused_instances():
        rows.append(("lscqp_fused.hip", "fused_%d_%d_%d_%d_%d" % (M, D, E, S, W),
                     ["-DLSCQP_M=%d" % M, "-DLSCQP_DIM=%d" % D, "-DLSCQP_ES=%d" % E, "-DLSCQP_NSLOT=%d" % S, "-DLSCQP_W=%d" % W] + fused_flags(M, D),
                     "LSCQP_EXTRA_F64_FLAGS", True))
    rows += [
        ("lscqp_api.hip", "api", [], "LSCQP_EXTRA_F64_FLAGS", False),
        ("lscpost.hip", "lscpost", [], None, False),
        # the mission record.  -Rpass-analysis=kernel-resource-usage puts the kernel's registers, scratch and LDS into the build log (a verbose
        # build prints it): the kernel is required to use no scratch
        ("lscrecord.hip", "lscrecord", ["-Rpass-analysis=kernel-resource-usage"], None, False),
        ("lscgoal.hip", "lscgoal", [], None, False),
        ("lscsfc.hip", "lscsfc", [], None, False),
        ("lscsfc_tp.hip", "lscsfc_tp", [], None, False),
        ("lscqp_comm.hip", "lscqp_comm", [], None, False),
        # (lscplan.hip includes lscobstacle.hip, the obstacles' motion: one object.  The remark puts obstacle_advance_kernel's registers,
        # scratch and LDS into the verbose build's log: the kernel is required to use no scratch)
        ("lscplan.hip", "lscplan", ["-Rpass-analysis=kernel-resource-usage"], None, False),
        ("lscgrid.hip", "lscgrid", [], None, False),
        # (the remark: generate_clsc_obstacle_kernel is required to use no scratch)
        ("lscgen.hip", "lscgen", ["-Rpass-analysis=kernel-resource-usage"], None, False),
        ("lscqp_generic.hip", "lscqp_generic", [], None, False),
        # -ffp-contract=on: a multiply-add is fused where the SOURCE writes a * b + c in one expression and nowhere else.  The default (fast) lets
        # the backend fuse across statements as the surrounding code happens to allow -- the kernel's instantiations (row formats, wavefronts
        # per QP, launch forms) then differ in the last bit, and the phase's results are required to be identical across all of them.
        # Its twin (LSCQP_DAS_FULL_SYNC) goes into liblscqp_sync.so in its place, beside the product's own objects (tests/test_race_twin.py)
        ("lscqp_das.hip", "lscqp_das", ["-ffp-contract=on"], None, True),
        # (-ffp-contract=on as the phase: the row formats' instantiations and the host twin then round alike wherever the source writes one expression)
        ("lscqp_prescreen.hip", "lscqp_prescreen", ["-ffp-contract=on"], None, False),
        ("lscqp_diag.hip", "lscqp_diag", [], None, False),
    ]
    return rows


def _stale(o, mtime):
    """Dependencies come from the compiler (-MD -MF <obj>.d): an object is stale when it or its depfile is missing, or this file or any
    file the depfile names is newer (a named file that is gone counts as newer)."""
    d = o + ".d"
    if not os.path.exists(o) or not os.path.exists(d):
        return True
    deps = open(d).read().replace("\\\n", " ").split(":", 1)[1].split()
    # The depfile names the tree it was written in.  A built tree that was copied elsewhere is judged by ITS files: the first name is the
    # unit's own source, <that tree>/csrc/<unit>, and every name under that directory (the ../../include ones too) is read under CSRC.
    was = os.path.dirname(deps[0]) if deps else CSRC
    if was != CSRC:
        deps = [CSRC + p[len(was):] if p.startswith(was + os.sep) else p for p in deps]
    t = os.path.getmtime(o)
    return any(mtime(p) > t for p in deps + [os.path.abspath(__file__)])


def commands(force=False):
    """The (object, command line) pairs build() would run, in its order; nothing is run."""
    seen = {}

    def mtime(p):
        if p not in seen:
            seen[p] = os.path.getmtime(p) if os.path.exists(p) else float("inf")
        return seen[p]

    out = []
    for src, name, flags, env, twin in units():
        for suffix, more in (("", []), ("_sync", ["-DLSCQP_DAS_FULL_SYNC"]))[:2 if twin else 1]:
            o = os.path.join(OBJ, name + suffix + ".o")
            if force or _stale(o, mtime):
                out.append((o, [HIPCC] + FLAGS + _env(env) + flags + more + ["-MD", "-MF", o + ".d", "-c", os.path.join(CSRC, src), "-o", o]))
    return out


def build(force=False, verbose=False, jobs=None):
    os.makedirs(OBJ, exist_ok=True)
    tasks = commands(force)
    if tasks:
        with ThreadPoolExecutor(max_workers=_workers(jobs)) as ex:
            for msg in ex.map(_run, [cmd for _, cmd in tasks]):
                if verbose and msg:
                    sys.stderr.write(msg)
    objs = [os.path.join(OBJ, name + ".o") for _, name, _, _, _ in units()]
    twin = {os.path.join(OBJ, name + ".o"): os.path.join(OBJ, name + "_sync.o") for _, name, _, _, has_twin in units() if has_twin}
    # work counters of every instance, read off its machine code (isa_work.py) -> one small generated host TU
    work_o = os.path.join(OBJ, "lscqp_work_table.o")
    inst_objs = [o for o in objs if os.path.basename(o).startswith("inst_")]
    objs.append(work_o)
    if force or _newer(work_o, inst_objs + [os.path.join(HERE, "isa_work.py"), os.path.abspath(__file__)]):
        _work_table(inst_objs, work_o, jobs)
        tasks.append("work table")
    if tasks or not os.path.exists(LIB):
        _run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs + ["-ldl", "-lpthread"])
    if tasks or not os.path.exists(SYNC_LIB):
        _run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", SYNC_LIB] + [twin.get(o, o) for o in objs] + ["-ldl", "-lpthread"])
    return LIB


def _work_table(inst_objs, work_o, jobs=None):
    import json
    import tempfile

    sys.path.insert(0, HERE)
    import isa_work

    def one(o):
        # reporting only (lscqp_instance_work): an instance whose machine code cannot be read (another ROCm layout, markers moved
        # or duplicated by the compiler) gets NO row -- lscqp_work_table_ then returns 1 and the API answers UNSUPPORTED for it --
        # and never stops the library from linking
        js = o[:-2] + ".work.json"
        try:
            if not _newer(js, [o, os.path.join(HERE, "isa_work.py")]):
                return json.load(open(js))
            with tempfile.TemporaryDirectory() as td:
                w = isa_work.of_object(o, td)
            json.dump(w, open(js, "w"))
            return w
        except Exception as ex:  # noqa: BLE001
            sys.stderr.write("build.py: warning: no work counters for %s (%s: %s)\n" % (os.path.basename(o), type(ex).__name__, str(ex)[:200]))
            return None

    with ThreadPoolExecutor(max_workers=_workers(jobs)) as ex:
        works = list(ex.map(one, inst_objs))
    src = os.path.join(OBJ, "lscqp_work_table.cpp")
    with open(src, "w") as f:
        f.write("// generated by lsc_dr_planner_amd/build.py from the instances' machine code (isa_work.py); per wavefront\n")
        f.write("struct Row { int M, D, E, S, W, X; double t[24]; };\nstatic const Row kRows[] = {\n")
        f.write("    {-1, -1, -1, -1, -1, -1, {0}},\n")  # (keeps the array non-empty when no instance could be read)
        for o, w in zip(inst_objs, works):
            if w is None:
                continue
            key = os.path.basename(o)[5:-2].split("_")
            # per section: instructions every wavefront runs (fma, other fp64, valu, lds), then the ones only SOME wavefronts run, summed
            # over those wavefronts (nested-dissection instances)
            vals = [w["%s_%s" % (a, b)] for a in ("iter", "last", "fixed")
                    for b in ("fma_f64", "other_f64", "valu", "lds", "partial_fma_f64", "partial_other_f64", "partial_valu", "partial_lds")]
            f.write("    {%s, {%s}},\n" % (", ".join(key), ", ".join(str(v) for v in vals)))
        f.write("};\nextern \"C\" int lscqp_work_table_(int M, int D, int E, int S, int W, int X, double* out24) {\n"
                "    for (const Row& r : kRows)\n        if (r.M == M && r.D == D && r.E == E && r.S == S && r.W == W && r.X == X) {\n"
                "            for (int i = 0; i < 24; i++) out24[i] = r.t[i];\n            return 0;\n        }\n    return 1;\n}\n")
    _run(["g++", "-O1", "-fPIC", "-c", src, "-o", work_o])


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
