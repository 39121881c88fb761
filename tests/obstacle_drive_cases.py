"""The scenario the obstacle-drive tests share (tests/test_obstacle_drives_cpu.py, _gpu.py): a six-entry table -- a straight obstacle, a
patrol, two chasers started 0.3 m apart with radius 0.2 (inside each other's Q* = 0.8), a gaussian obstacle whose history ends before the
flight does, and a plain HELD entry filled with a sentinel that nothing may touch -- and a mission of three agents of which agent 0, the
first chaser's target, flies a circle.  `twins` puts the two chasers at ONE start with one goal: they stay on top of each other, which is the
reference's `dist < 1e-5` skip.  The expected tables come from the restatement alone (tests/obstacle_drive_reference.py)."""
import numpy as np

from tests import obstacle_drive_reference as D

N_TOTAL, K = 3, 40
STRAIGHT, PATROL, CHASER_A, CHASER_B, GAUSS, HELD = range(6)


def specs(twins=False):
    b_start = [0.0, 0.0, 1.0] if twins else [0.3, 0.0, 1.0]
    rng = np.random.default_rng(5)
    history = rng.normal(0.0, 1.0, (60, 3))  # 6 s of a flight of 8 s (6 s at time_step 0.15): the history ends
    norm = np.sqrt((history ** 2).sum(1))
    history[norm > 1.2] *= (1.2 / norm[norm > 1.2])[:, None]
    return [dict(type="straight", start=[-1.0, 0.6, 1.0], goal=[2.0, 0.4, 1.0], size=0.2, speed=0.5, max_acc=1.0, downwash=1.0),
            dict(type="patrol", waypoints=[[1.0, -1.0, 1.0], [1.0, 1.5, 1.2]], size=0.25, speed=0.4, max_acc=1.0, downwash=1.0),
            dict(type="chasing", start=[0.0, 0.0, 1.0], size=0.2, max_vel=0.5, max_acc=1.5, gamma_target=1.0, gamma_obs=1.0, downwash=1.5,
                 **(dict(goal=[1.5, 1.0, 1.0]) if twins else dict(target_agent=0))),
            dict(type="chasing", start=b_start, size=0.2, max_vel=0.5, max_acc=1.5, gamma_target=1.0, gamma_obs=1.0, downwash=1.5,
                 goal=[1.5, 1.0, 1.0]),
            dict(type="gaussian", start=[-2.0, -2.0, 1.5], size=0.3, initial_vel=[0.3, 0.1, 0.0], max_vel=0.45, stddev_acc=1.0, max_acc=1.2,
                 acc_update_cycle=0.0, downwash=1.0, acc_history=history),
            dict(type="real", start=[9.0, 9.0, 9.0], size=0.33, max_acc=6.5, downwash=4.5)]


def state_at(r):
    """[N_TOTAL][9]: agent 0 on a circle of radius 1.5 m (point3d: float32 held in double), the others parked."""
    st = np.zeros((N_TOTAL, 9))
    st[0, :3] = np.float32([1.5 * np.cos(0.15 * r), 1.5 * np.sin(0.15 * r), 1.0])
    st[1, :3], st[2, :3] = [5.0, 5.0, 1.0], [-5.0, 5.0, 1.0]
    return st


def table_at_reset(api, models):
    """The table as lscqp_plan_reset leaves it -- every entry at `start` with zero velocity -- with the plain HELD entry a sentinel."""
    t = np.zeros(len(models), api.OBSTACLE_DTYPE)
    t["position"] = np.float32(models["start"])
    t["radius"], t["downwash"], t["max_acc"] = models["radius"], models["downwash"], models["max_acc"]
    t["velocity"][HELD], t["type"][HELD], t["reserved"][HELD] = (7.0, -7.0, 7.5), 0x5A5A5A5A, 0x3C3C3C3C
    return t


def scenario(api, twins=False):
    s = specs(twins)
    models = api.obstacle_model_prepare(api.obstacle_models(s))
    drives, history = api.obstacle_drives(s, N_TOTAL)
    return dict(models=models, drives=drives, history=history, table0=table_at_reset(api, models))


def reference_flight(sc, time_step, replans=range(K)):
    """The table behind (drive, advance) of every replan in `replans`, from the restatement; and the branches it took."""
    D.counts.clear()
    table, out = sc["table0"].copy(), []
    for r in replans:
        D.drive_table(sc["models"], sc["drives"], sc["history"], table, state_at(r), r, time_step)
        D.advance_table(sc["models"], table, r, time_step)
        out.append(table.copy())
    return out, dict(D.counts)
