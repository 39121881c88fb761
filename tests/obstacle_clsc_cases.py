"""Inputs for generateCLSC's rows of NON-AGENT obstacles (csrc/lscgen.hip: generate_clsc_obstacle_kernel) -- TEST INFRASTRUCTURE.

Three kinds of pack, all with one obstacle per agent (n_dyn = 1) and the fields the device runner and the references read:
  pack_static   the constructed hulls of tests/lscgen_cases.py on segments 0 .. M-2 against a static obstacle (velocity 0: its six
                predicted points are its position), so that the rows are stated by construction; the last segment is a plain
                segment-to-segment case
  pack_moving   random float32 trajectories against obstacles with velocity != 0 (nothing is stated by construction: held to the
                restatement and to the agent generator)
  pack_segseg   the 240 segment pairs of tests/golden/segseg.json on the last segment
A 2-D pack lies in the plane z = Z_2D = 0.6 like the reference's missions; pack_static passes no obstacle goal points, so its last segment
separates (obstacle -> the origin, which is off that plane) from (agent -> its goal): the record's normal has a z component there, and
the packed row must not (n_z = 0, b = d + n_x p_x + n_y p_y: the 2-D QP's row, src/traj_optimizer.cpp:414-421).
as_agent_pairs turns a pack into the equivalent AGENT pair of tests/lscgen_cases.pack_pairs' shape: the neighbour flies the obstacle's
predicted points, has its radius and downwash, the planning agent's downwash is 1 (which turns downwashBetween's agent formula into the
non-agent one) and goal_all[neighbour] is the obstacle's goal point."""
import numpy as np

from tests import lscgen_cases as LC
from tests import obstacle_rows_reference as RR

DT = 0.2
THRESHOLD = 3.0  # obs_downwash_threshold
Z_2D = float(np.float32(0.6))  # world/z_2d of the reference's launch files: the plane of a 2-D pack, OFF the origin that an obstacle's goal defaults to
TABLE_DTYPE = [("position", "f8", 3), ("velocity", "f8", 3), ("radius", "f8"), ("downwash", "f8"), ("max_acc", "f8"), ("type", "i4"), ("reserved", "i4")]


def _groups(cases, size):
    order = sorted(range(len(cases)), key=lambda i: (cases[i]["dwk"], cases[i]["fb"] == "zero", cases[i]["obs_max"]))
    groups, cur = [], []
    for i in order:
        key = (cases[i]["dwk"], cases[i]["fb"])
        if cur and (len(cur) == size or (cases[cur[0]]["dwk"], cases[cur[0]]["fb"]) != key):
            groups.append(cur)
            cur = []
        cur.append(i)
    groups.append(cur)
    return groups


def pack_static(cases, M, dim, tall=False, seed=0):
    """One hull per (agent, segment < M-1).  The pairs are tests/lscgen_cases.py's: OBSTACLE_PAIRS give downwashBetween exactly 1 or 2, TALL
    2.5 with a type-0 obstacle above the threshold.  3-D tall: the z of the agent's points is noise, which the hull drops and, the normal
    being planar, the margins do not see.  2-D: every z is Z_2D (generateCLSC does not drop z in 2-D, it relies on this)."""
    assert M >= 2
    rng = np.random.default_rng(seed)
    groups = _groups(cases, M - 1)
    N = len(groups)
    traj, radius, goal = np.zeros((N, M, 6, 3)), np.zeros(N), np.zeros((N, 3))
    table = np.zeros(N, dtype=TABLE_DTYPE)
    slot = -np.ones((N, M), dtype=np.int64)
    dws = np.zeros(N)
    for a, g in enumerate(groups):
        dwk = cases[g[0]]["dwk"] if dim == 3 else 1
        if tall:
            r_own, r_ob, dw_ob, dw = LC.TALL
            typ = 0
        else:
            r_own, r_ob, dw_ob = LC.OBSTACLE_PAIRS[dwk][a % 2]
            dw, typ = float(dwk), (0 if dw_ob <= THRESHOLD else 1)  # (type 1 keeps a downwash-5 obstacle out of the tall rule)
        top = min(cases[i]["obs_max"] for i in g)
        k = int(top / 0.25)
        pos = rng.integers(-k, k + 1, 3) * 0.25 if k > 0 else np.zeros(3)
        if dim == 2:
            pos[2] = Z_2D
        radius[a] = r_own
        table[a]["position"], table[a]["radius"], table[a]["downwash"], table[a]["max_acc"], table[a]["type"] = pos, r_ob, dw_ob, 1.5, typ
        dws[a] = RR.downwash_between(r_own, table[a])
        assert dws[a] == dw or dim == 2
        zscale = dw if dim == 3 else 1.0
        for m in range(M - 1):
            ci = g[m] if m < len(g) else g[0]
            if m < len(g):
                slot[a, m] = ci
            rel = cases[ci]["rel"].copy()
            if tall and dim == 3:
                rel[:, 2] = rng.integers(-8, 9, 6) * 0.25
            elif dim == 2:
                rel[:, 2] = 0.0
            own = pos + rel * np.array([1.0, 1.0, 1.0 if tall else zscale])
            traj[a, m] = own
            assert LC._exact32(own), cases[ci]["name"]
            d32 = (np.float32(own) - np.float32(pos)).astype(np.float64)
            assert np.array_equal(d32[:, :2], cases[ci]["rel"][:, :2]), cases[ci]["name"]
            if dim == 3 and not tall:
                dz = (np.float32(own[:, 2]) / np.float32(dw) - np.float32(pos[2]) / np.float32(dw)).astype(np.float64)
                assert np.array_equal(dz, cases[ci]["rel"][:, 2]), cases[ci]["name"]
        last = pos + np.array([1.5, -0.75, 0.5 if dim == 3 else 0.0])
        traj[a, M - 1] = last
        goal[a] = last + np.array([-0.5, 2.0, 0.25 if dim == 3 else 0.0])
    return dict(N=N, traj=traj, radius=radius, goal=goal, table=table, ids=np.arange(N, dtype=np.int32).reshape(N, 1), slot=slot, dw=dws, M=M,
                dim=dim, tall=tall, obstacle_goal=None)


def expected_static(cases, pk, normals):
    """(N, M, 6, 4): the constructed rows on the hull segments, NaN on the last one"""
    N, M = pk["N"], pk["M"]
    want = np.full((N, M, 6, 4), np.nan)
    for a in range(N):
        for m in range(M - 1):
            ci = pk["slot"][a, m]
            if ci < 0:
                continue
            c = cases[ci]
            if pk["tall"] or pk["dim"] == 2:
                c = dict(c, rel=c["rel"] * np.array([1.0, 1.0, 0.0]))
            pos = np.tile(pk["table"][a]["position"], (6, 1))
            want[a, m] = LC.expected_rows(c, normals[ci], pos, pk["radius"][a] + pk["table"][a]["radius"], pk["dw"][a], None, "clsc", pk["dim"])
    return want


def pack_moving(M, dim, n=24, seed=1, with_tall=True):
    """Random float32 trajectories 1 .. 3 m from obstacles that move at up to 1 m/s; radii and downwashes from a short list whose
    products are exact in double.  Every fourth obstacle is tall when with_tall (3-D: planar normal, z of the agent's points free)."""
    rng = np.random.default_rng(seed)
    traj, radius, goal = np.zeros((n, M, 6, 3)), np.zeros(n), np.zeros((n, 3))
    table = np.zeros(n, dtype=TABLE_DTYPE)
    ogoal = np.zeros((n, 3))
    f = lambda x: np.float32(x).astype(np.float64)  # noqa: E731
    for a in range(n):
        tall = with_tall and a % 4 == 3
        pos = f(rng.uniform(-4, 4, 3))
        vel = f(rng.uniform(-1, 1, 3))
        if dim == 2:
            pos[2], vel[2] = Z_2D, 0.0
        radius[a] = (0.15, 0.25, 0.5)[a % 3]
        table[a]["position"], table[a]["velocity"] = pos, vel
        table[a]["radius"], table[a]["downwash"] = (0.25, 0.5, 0.75)[(a // 3) % 3], (4.0 if tall else (1.0, 2.0, 3.0)[a % 3])
        table[a]["max_acc"], table[a]["type"] = 1.5, 0
        pred = RR.predicted_points(M, DT, pos, vel).astype(np.float64)
        dirn = rng.normal(size=3)
        if dim == 2:
            dirn[2] = 0.0
        dirn /= np.linalg.norm(dirn)
        for m in range(M):
            off = dirn * rng.uniform(1.0, 3.0) + rng.uniform(-0.4, 0.4, (6, 3))
            if dim == 2:
                off[:, 2] = 0.0
            traj[a, m] = f(pred[m] + off)
        goal[a] = f(traj[a, M - 1, 5] + rng.uniform(-2, 2, 3) * np.array([1.0, 1.0, 0.0 if dim == 2 else 1.0]))
        ogoal[a] = f(pred[M - 1, 5] + rng.uniform(-2, 2, 3) * np.array([1.0, 1.0, 0.0 if dim == 2 else 1.0]))
    return dict(N=n, traj=traj, radius=radius, goal=goal, table=table, ids=np.arange(n, dtype=np.int32).reshape(n, 1), M=M, dim=dim,
                obstacle_goal=ogoal, tall_mask=np.array([RR.is_tall(table[a], THRESHOLD) for a in range(n)]))


def pack_segseg(g, M=2):
    """Predicted last point l1s (velocity 0), obstacle goal l1e, own last point l2s, agent goal l2e, downwash 1 (as tests/test_lscmode.py
    packs the agent branch); segment 0 is a separated hull of no interest."""
    N = len(g)
    traj, goal, ogoal = np.zeros((N, M, 6, 3)), np.zeros((N, 3)), np.zeros((N, 3))
    table = np.zeros(N, dtype=TABLE_DTYPE)
    for a, c in enumerate(g):
        traj[a, :, :] = np.float32(c["l2s"])
        if M > 1:
            traj[a, 0] += 16.0
        table[a]["position"] = np.float32(c["l1s"])
        goal[a], ogoal[a] = np.float32(c["l2e"]), np.float32(c["l1e"])
    table["radius"], table["downwash"], table["max_acc"], table["type"] = 0.15, 1.0, 1.5, 0
    return dict(N=N, traj=traj, radius=np.full(N, 0.15), goal=goal, table=table, ids=np.arange(N, dtype=np.int32).reshape(N, 1), M=M, dim=3,
                obstacle_goal=ogoal)


def as_agent_pairs(pk):
    N, M = pk["N"], pk["M"]
    traj = np.zeros((2 * N, M, 6, 3))
    traj[:N] = pk["traj"]
    for a in range(N):
        traj[N + a] = RR.predicted_points(M, DT, pk["table"][a]["position"], pk["table"][a]["velocity"]).astype(np.float64)
    og = np.zeros((N, 3)) if pk["obstacle_goal"] is None else pk["obstacle_goal"]
    return dict(N=N, M=M, dim=pk["dim"], traj=traj, nbr=(N + np.arange(N, dtype=np.int32)).reshape(N, 1),
                radius=np.concatenate([pk["radius"], pk["table"]["radius"]]), downwash=np.concatenate([np.ones(N), pk["table"]["downwash"]]),
                goal_all=np.concatenate([pk["goal"], og]))


def restatement(oracle, pk, records=False):
    """(N, M, 6, 4) rows of tests/obstacle_rows_reference.py; records=True: also the record normals (N, M, 3), z / downwash included"""
    from tests import hull_reference as R

    out, nrm = np.zeros((pk["N"], pk["M"], 6, 4)), np.zeros((pk["N"], pk["M"], 3))
    for a in range(pk["N"]):
        og = None if pk["obstacle_goal"] is None else pk["obstacle_goal"][a]
        out[a], rec = RR.clsc_obstacle_rows(oracle, R, pk["M"], pk["dim"], DT, pk["traj"][a], pk["goal"][a], float(pk["radius"][a]), pk["table"][a], THRESHOLD,
                                            og, records=True)
        nrm[a] = rec[1]
    return (out, nrm) if records else out


def agent_oracle_rows(oracle, pk):
    """oracle.generate_constraints(CLSC) on the equivalent agent pair, its LSC records (p, nrm, d) turned into rows as the QP of the pack's
    dimension reads them: n_k for k < dim (0 beyond), b = d + sum over k < dim of n_k p_k.  (N, M, 6, 4), and the record normals (N, M, 3)."""
    pr = as_agent_pairs(pk)
    L = oracle.generate_constraints(1, pr["traj"], pr["nbr"], pr["radius"], pr["downwash"], pr["goal_all"], dim=pk["dim"])[:, 0]
    keep = np.array([1.0, 1.0, 1.0 if pk["dim"] == 3 else 0.0])
    n = L["nrm"] * keep
    return np.concatenate([n, (L["d"] + (n * L["p"]).sum(-1))[..., None]], axis=-1), L["nrm"][:, :, 0]


# ---- device runner ---------------------------------------------------------------------------------------------------------------
def param(api):
    return api.ObstacleParam(1.0, 0.75, THRESHOLD, 0.1, 0, 0)


def run_device(api, pk, mode=None, rows_f32=False, goals="pack", n_obs_total=1, slot0=0, first_agent=0, ids=None, raw=False, n_agents=None):
    """One lscqp_generate_obstacle_rows_device launch over a pack: (N, M, 6, 4) rows of slot `slot0`, or with raw=True the whole buffer's
    bytes (filled with 0xFF beforehand).  goals: "pack" = the pack's obstacle goal table (None where the pack has none), None = NULL,
    "zeros" = an explicit all-zero table.  first_agent > 0: the local agents are the pack's [first_agent, first_agent + n_agents)."""
    import torch

    dev = torch.device("cuda", 0)
    kw = dict(row_format=api.ROWS_F32) if rows_f32 else {}
    N, M = pk["N"], pk["M"]
    # (no handle admits M = 1: there the launch itself, lscqp_generate_clsc_obstacles_raw_, as tests/test_lscgen.py reaches the agent kernel)
    sol = api.Solver(api.make_desc(M=M, dim=pk["dim"], dt=DT, world_min=(-40, -40, -40), world_max=(40, 40, 40), **kw)) if M >= 2 else None
    n = N - first_agent if n_agents is None else n_agents
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    item = 16 if rows_f32 else 32
    ids = pk["ids"][first_agent:first_agent + n] if ids is None else ids
    n_dyn = ids.shape[1]
    d_rows = torch.full((n * n_obs_total * M * 6 * item,), 0xFF, dtype=torch.uint8, device=dev)
    table = np.zeros(N, api.OBSTACLE_DTYPE)
    for f in ("position", "velocity", "radius", "downwash", "max_acc", "type"):
        table[f] = pk["table"][f]
    og = pk.get("obstacle_goal") if goals == "pack" else (np.zeros((N, 3)) if goals == "zeros" else None)
    hdr = np.zeros(n, api.HEADER_DTYPE)
    hdr["amax"] = 2.0
    t = [up(pk["traj"]), up(ids), up(table), None if og is None else up(og), up(pk["radius"]), up(pk["goal"][first_agent:first_agent + n])]
    if sol is None:
        import ctypes as C

        assert mode in (None, api.GEN_CLSC)
        fn = api.lib().lscqp_generate_clsc_obstacles_raw_
        fn.restype = C.c_int
        fn.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_int64, C.c_int32, C.c_int64] + [C.c_void_p] * 6 + [C.c_int, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        p = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
        rc = fn(M, pk["dim"], DT, THRESHOLD, n, n_dyn, first_agent, *[p(x) for x in t], int(rows_f32), n_obs_total, slot0, p(d_rows),
                C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
    else:
        sol.generate_obstacle_rows_device(api.GEN_CLSC if mode is None else mode, param(api), n, n_dyn, first_agent, *t,
                                          up(hdr) if mode == api.GEN_LSC else None, d_rows, n_obs_total, slot0)
    torch.cuda.synchronize()
    buf = d_rows.cpu().numpy()
    if sol is not None:
        sol.close()
    if raw:
        return buf
    return LC.rows_array(buf, api, rows_f32, (n, n_obs_total, M, 6))[:, slot0]
