"""Inputs of the obstacle record's tests (tests/record_obstacles_reference.py restates it): a hand table whose expected output is written
out by construction, and random flights drawn from a few values so that ties, +inf, NaN and the two sides of 1.0 come up at every size."""
import numpy as np

from tests import record_obstacles_reference as ROR

INF, NAN = float("inf"), float("nan")
BELOW = float(np.nextafter(1.0, 0.0))  # the largest double below 1.0: counted in below_one; 1.0 itself is not
NONE = (INF, -1, -1)                   # an agent that compared nothing (lscqp_safety_obstacles_device: +inf, -1)


def hand_table():
    """Three missions -- agents 0-2, 3-4, 5-6 -- and four replans; mission 1 freezes at replan 1 (its replans 2 and 3 hold ratios that
    would lower every figure of it).  Returns (offsets, steps, missions, agents): steps as ROR.flight takes them, the last two the expected
    structs as lists of dicts.

    mission 0  r0: agents 1 and 2 tie at 1.5 -> agent 1 (the smaller id).  r1: agent 0 ties the mission's 1.5 -> replan 0 keeps it; agent 1
               ties its own 1.5 -> its entry stays at replan 0.  r2: a NaN (not compared), 1.0 (not below one) and BELOW (below one, the
               new minimum: agent 2).  r3: agents 1 and 2 tie BELOW, the mission's figure -> replan 2 keeps it; agent 2 keeps replan 2.
               compared 3 + 3 + 2 + 3, below_one 0 + 0 + 1 + 2.
    mission 1  agent 3 compares nothing; agent 4: 0.9, then 0.8; frozen from replan 2 on.
    mission 2  agent 5 at +inf throughout; agent 6: +inf, NaN, 1.0, 1.0 -> replan 2 keeps the tie; nothing below one."""
    offsets = [0, 3, 5, 7]
    frozen = (0.05, 0, 0)
    rows = [
        [(2.0, 0, 0), (1.5, 1, 1), (1.5, 0, 1), NONE, (0.9, 1, 1), NONE, NONE],
        [(1.5, 1, 0), (1.5, 0, 0), (3.0, 1, 1), NONE, (0.8, 0, 0), NONE, (NAN, 0, 0)],
        [(NAN, 1, 1), (1.0, 1, 0), (BELOW, 0, 1), frozen, frozen, NONE, (1.0, 1, 1)],
        [(2.5, 0, 0), (BELOW, 0, 0), (BELOW, 1, 0), frozen, frozen, NONE, (1.0, 0, 0)],
    ]
    finished = [[0, 0, 0], [0, 0, 0], [0, 1, 0], [0, 1, 0]]
    replans = [[0, 0, 0], [1, 1, 1], [2, 2, 2], [3, 2, 3]]
    steps = list(zip(rows, finished, replans))
    missions = [dict(safety_ratio_obs=BELOW, replan=2, agent=2, obstacle=0, sample=1, below_one=3, compared=11),
                dict(safety_ratio_obs=0.8, replan=1, agent=4, obstacle=0, sample=0, below_one=2, compared=2),
                dict(safety_ratio_obs=1.0, replan=2, agent=6, obstacle=1, sample=1, below_one=0, compared=2)]
    agents = [dict(safety_ratio_obs=1.5, replan=1, obstacle=1, sample=0, reserved=0),
              dict(safety_ratio_obs=BELOW, replan=3, obstacle=0, sample=0, reserved=0),
              dict(safety_ratio_obs=BELOW, replan=2, obstacle=0, sample=1, reserved=0),
              dict(safety_ratio_obs=INF, replan=-1, obstacle=-1, sample=-1, reserved=0),
              dict(safety_ratio_obs=0.8, replan=1, obstacle=0, sample=0, reserved=0),
              dict(safety_ratio_obs=INF, replan=-1, obstacle=-1, sample=-1, reserved=0),
              dict(safety_ratio_obs=1.0, replan=2, obstacle=1, sample=1, reserved=0)]
    return offsets, steps, missions, agents


VALUES = np.array([0.5, 0.75, BELOW, 1.0, 1.25, 2.0, INF, NAN])


def random_figures(rng, n, dtype, n_dyn=3, n_samples=2):
    """One replan's lscqp_safety_obs for n agents: ratios drawn from VALUES (ties within a replan and across replans at every size), the
    obstacle and the sample random -- so that WHICH agent or replan won a tie shows in them -- and (-1, -1) beside +inf."""
    out = np.zeros(n, dtype)
    out["safety_ratio_obs"] = VALUES[rng.integers(0, len(VALUES), n)]
    none = np.isposinf(out["safety_ratio_obs"])
    out["closest_obstacle"] = np.where(none, -1, rng.integers(0, n_dyn, n))
    out["sample"] = np.where(none, -1, rng.integers(0, n_samples, n))
    return out


def figures_of(rows, dtype):
    """A replan of the hand table as lscqp_safety_obs records."""
    out = np.zeros(len(rows), dtype)
    for a, (v, o, s) in enumerate(rows):
        out[a] = (v, o, s)
    return out


def triples(figures):
    return [(float(f["safety_ratio_obs"]), int(f["closest_obstacle"]), int(f["sample"])) for f in figures]


def same_structs(got, want):
    """Field for field, NaN-free by construction (a NaN is never taken): the bytes."""
    return got.dtype == want.dtype and got.tobytes() == want.tobytes()


__all__ = ["ROR", "hand_table", "random_figures", "figures_of", "triples", "same_structs", "BELOW", "INF", "NAN", "VALUES"]
