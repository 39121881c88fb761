"""What the tests of a mission's own obstacles share (include/lscqp.h, "a mission's own obstacles"; tests/test_mission_obstacles_cpu.py,
_gpu.py, _plan_gpu.py): mission-major tables of every model and drive kind for the kernels alone, and forest10 cut into missions of at most
six agents, each with obstacles of its own, for the chain.  Nothing here touches a device."""
import numpy as np

from tests import waypoint_cases as WC

TIME_STEP = 0.2
CLOCKS = (0, 7, 400)  # mission k's clock before the launch: different per mission, so a kernel that reads one word for all is wrong
# per-mission counts of the kernel tests: every value of {0, 1, 63, 64, 65} -- none, one, one short of the 64 threads, exactly them, one more
# (the strided loop) -- in front of, between and behind other missions, for K = 1, 2, 3
SHAPES = [(65,), (0,), (1, 64), (63, 0), (0, 65, 1), (64, 63, 65), (1, 0, 0)]


def offsets(counts):
    off = np.zeros(len(counts) + 1, np.int32)
    off[1:] = np.cumsum(counts)
    return off


# ---- the kernels alone -------------------------------------------------------------------------------------------------------------------

def advance_specs(n, seed):
    """n mission-file entries cycling through the four model kinds (straight, patrol, spin, held), seeded."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        p, q = rng.uniform(-3, 3, 3), rng.uniform(-3, 3, 3)
        common = dict(size=float(rng.uniform(0.1, 0.4)), speed=float(rng.uniform(0.2, 1.0)), max_acc=float(rng.uniform(0.5, 2.0)), downwash=float(rng.uniform(1, 2)))
        if i % 4 == 0:
            out.append(dict(type="straight", start=p.tolist(), goal=q.tolist(), **common))
        elif i % 4 == 1:
            out.append(dict(type="patrol", waypoints=[p.tolist(), q.tolist(), rng.uniform(-3, 3, 3).tolist()], **common))
        elif i % 4 == 2:
            out.append(dict(type="spin", start=p.tolist(), axis=[0.0, 0.0, 1.0] + (rng.uniform(-1, 1, 3) + [0, 0, 2]).tolist(), **common))
        else:
            out.append(dict(type="real", start=p.tolist(), **common))
    return out


def drive_specs(n, seed, n_total, history_len):
    """n entries cycling through straight (no drive), a chaser after an agent, a chaser to a goal point, a gaussian obstacle and a plain
    HELD entry, on a lattice of 0.5 m pitch: with radius 0.2 (Q* = 0.8) every chaser has neighbours inside its avoiding distance."""
    rng = np.random.default_rng(seed)
    side = max(1, int(np.ceil(n ** (1 / 3))))
    cell = np.array([(i, j, k) for i in range(side) for j in range(side) for k in range(side)][:n], np.float64).reshape(n, 3)
    start = 0.5 * cell + rng.uniform(-0.05, 0.05, (n, 3))
    out = []
    for i in range(n):
        s = start[i].tolist()
        if i % 5 == 0:
            out.append(dict(type="straight", start=s, goal=rng.uniform(-3, 3, 3).tolist(), size=0.2, speed=0.5, max_acc=1.0, downwash=1.0))
        elif i % 5 in (1, 2):
            tgt = dict(target_agent=int(rng.integers(n_total))) if i % 5 == 1 and n_total else dict(goal=rng.uniform(-1, 4, 3).tolist())
            out.append(dict(type="chasing", start=s, size=0.2, max_vel=0.8, max_acc=2.0, gamma_target=0.7, gamma_obs=1.5, downwash=1.0, **tgt))
        elif i % 5 == 3:
            out.append(dict(type="gaussian", start=s, size=0.2, initial_vel=rng.uniform(-0.2, 0.2, 3).tolist(), max_vel=0.45, max_acc=1.2,
                            acc_update_cycle=0.1, downwash=1.0, acc_history=np.zeros((history_len, 3))))
        else:
            out.append(dict(type="real", start=s, size=0.2, max_acc=1.0, downwash=1.0))
    return out


def shared_history(n, seed=11):
    rng = np.random.default_rng(seed)
    h = rng.normal(0.0, 1.0, (n, 3))
    norm = np.sqrt((h ** 2).sum(1))
    h[norm > 1.2] *= (1.2 / norm[norm > 1.2])[:, None]
    return h


def drive_tables(api, counts, n_total, seed=3, history_len=120):
    """(models, drives, history) of a mission-major table: every gaussian obstacle of every mission reads the SAME slice [0, history_len) of
    one history table."""
    specs = [s for k, c in enumerate(counts) for s in drive_specs(c, seed + k, n_total, history_len)]
    models = api.obstacle_model_prepare(api.obstacle_models(specs)) if specs else np.zeros(0, api.OBSTACLE_MODEL_DTYPE)
    drives, _ = api.obstacle_drives(specs, n_total) if specs else (np.zeros(0, api.OBSTACLE_DRIVE_DTYPE), None)
    g = drives["kind"] == api.DRIVE_GAUSSIAN
    drives["history_first"][g], drives["history_len"][g] = 0, history_len
    return models, drives, shared_history(history_len)


def neighbours_across_missions(api):
    """Two missions of two entries each: a chaser and a straight obstacle far away.  The two chasers start 0.3 m apart with radius 0.2, inside
    each other's Q* = 0.8 -- each within avoiding distance of an obstacle of the OTHER mission and of none of its own."""
    def mission(x):
        return [dict(type="chasing", start=[x, 0.0, 1.0], size=0.2, max_vel=0.5, max_acc=1.5, gamma_target=1.0, gamma_obs=1.0, downwash=1.5, goal=[1.5, 1.0, 1.0]),
                dict(type="straight", start=[x, 6.0, 1.0], goal=[x, 9.0, 1.0], size=0.2, speed=0.5, max_acc=1.0, downwash=1.0)]

    specs = mission(0.0) + mission(0.3)
    models = api.obstacle_model_prepare(api.obstacle_models(specs))
    drives, _ = api.obstacle_drives(specs, 0)
    return models, drives, offsets((2, 2))


def table_at_reset(api, models, fill=0x5A):
    """The table as lscqp_plan_reset leaves it, every field the reset does not know a sentinel: the kernels write whole entries of the models
    they move and no byte of the others."""
    t = np.frombuffer(bytes([fill]) * (len(models) * api.OBSTACLE_DTYPE.itemsize), api.OBSTACLE_DTYPE).copy()
    t["position"] = np.float32(models["start"])
    t["velocity"] = 0.0
    t["radius"], t["downwash"], t["max_acc"] = models["radius"], models["downwash"], models["max_acc"]
    return t


def agent_states(n_total, seed=9):
    st = np.zeros((n_total, 9))
    st[:, :3] = np.float32(np.random.default_rng(seed).uniform(-1, 4, (n_total, 3)))
    return st


# ---- the safety figures by ids -----------------------------------------------------------------------------------------------------------

SAFETY_AGENTS = (1, 63, 64, 65, 257)  # one, around the wavefront, and more than the 256 lanes of a workgroup
N_SLOTS = 5
REAL, TWIN_A, TWIN_B = 2, 4, 6  # table entry 2 is a REAL obstacle; entries 4 and 6 are one obstacle twice: an exact tie
# the rows the agents cycle through: -1 in front of, between and behind live ids, the tie with the HIGHER table index in the LOWER slot, the
# REAL entry, a row of one id, and a row that names nothing
ID_ROWS = np.array([[-1, 3, 0, -1, -1], [0, -1, 5, -1, 1], [TWIN_B, TWIN_A, -1, -1, -1], [-1, -1, TWIN_B, 1, TWIN_A], [REAL, -1, 3, -1, -1],
                    [REAL, -1, -1, -1, -1], [-1, -1, -1, -1, 5], [-1, -1, -1, -1, -1], [6, 5, 3, 1, 0]], np.int32)


def safety_case(api, n, M=5, dim=3, seed=4):
    """n agents with seeded plans in a 4 m box, seven obstacles among them; agent a reads row a % len(ID_ROWS)."""
    rng = np.random.default_rng(seed + n)
    x = rng.uniform(0.0, 4.0, (n, dim, 1, 1)) + rng.uniform(-0.3, 0.3, (n, dim, M, 6))
    table = np.zeros(7, api.OBSTACLE_DTYPE)
    table["position"] = np.float32(rng.uniform(0.0, 4.0, (7, 3)))
    table["radius"], table["downwash"], table["max_acc"] = rng.uniform(0.1, 0.4, 7), rng.uniform(1.0, 2.5, 7), 1.0
    table[TWIN_B] = table[TWIN_A]
    table["type"][REAL] = api.OBSTACLE_REAL
    ids = ID_ROWS[np.arange(n) % len(ID_ROWS)].copy()
    return dict(x=np.ascontiguousarray(x.reshape(n, -1)), radius=rng.uniform(0.1, 0.2, n), downwash=rng.uniform(1.0, 2.5, n), table=table, ids=ids)


# ---- the chain: forest10 cut into missions -----------------------------------------------------------------------------------------------

N_OBS = 7        # row slots per agent: two obstacle slots and the five other agents of the largest mission
N_REPLANS = 30


def forest_missions(sizes):
    """forest10's first sum(sizes) agents as consecutive missions: (world, offsets, starts, goals)."""
    W = WC.forest10()
    n = sum(sizes)
    assert n <= len(W["starts"]) and max(sizes) <= 6
    off = np.zeros(len(sizes) + 1, np.int64)
    off[1:] = np.cumsum(sizes)
    return W, off, np.array(W["starts"], float)[:n], np.array(W["goals"], float)[:n]


def straight_and_chaser(z, k, target):
    """Mission k's own pair: a straight obstacle across the forest and a chaser after `target` (an agent id), both in the mission's plane and
    placed per mission, so that no two missions have the same obstacles."""
    y = -2.0 + 1.5 * k
    return [dict(type="straight", start=[2.5 - k, y, z], goal=[-2.5 + k, -y, z], size=0.15, speed=0.3, max_acc=1.0, downwash=1.0),
            dict(type="chasing", start=[4.8 - 0.4 * k, 4.8, z], size=0.1, max_vel=0.3, max_acc=1.0, gamma_target=1.0, gamma_obs=1.0, downwash=1.0,
                 target_agent=int(target))]


def unequal_specs(z):
    """Counts (2, 0, 1): mission 0 a straight obstacle and a patrol, mission 1 nothing, mission 2 a straight obstacle."""
    return [[dict(type="straight", start=[2.0, -1.0, z], goal=[-2.0, 1.0, z], size=0.15, speed=0.3, max_acc=1.0, downwash=1.0),
             dict(type="patrol", waypoints=[[-2.5, -1.5, z], [2.5, -1.5, z]], size=0.15, speed=0.3, max_acc=1.0, downwash=1.0)],
            [],
            [dict(type="straight", start=[-2.0, 2.0, z], goal=[2.0, -2.0, z], size=0.2, speed=0.25, max_acc=1.0, downwash=1.0)]]
