"""The obstacle record restated in plain Python (include/lscqp.h, "the obstacle record"): each mission's, and each agent's, least
agent-obstacle safety ratio over a flight -- the reference's `if (safety_ratio_obs > current)` (src/multi_sync_simulator.cpp:527-557)
applied replan after replan and, within a replan, agent after agent in id order.  It shares nothing with the kernel: scalar loops over
Python floats.  The arithmetic is DEFINED here:

  per replan r (the mission's own count, `replans` of its record BEFORE the replan), for every mission whose record is not finished
  before the replan, for every agent a of the mission in ascending GLOBAL id, with v = safety_obs[a].safety_ratio_obs:
    - the agent's entry takes (v, r, closest_obstacle, sample) if v < entry (strict: an earlier replan keeps a tie, a NaN never enters);
    - compared += 1 if v is finite; below_one += 1 if v < 1.0 (strict);
    - the replan's minimum takes (v, a, closest_obstacle, sample) if v < minimum (strict: the smallest id keeps a tie), from +inf;
  then the mission's figure takes the replan's minimum, with r, if it is strictly smaller (an earlier replan keeps a tie).
"""
import math

INF = float("inf")


def cleared(offsets):
    """(missions, agents) as lscqp_record_reset leaves them: lists of dicts with the structs' field names."""
    K, n = len(offsets) - 1, int(offsets[-1])
    missions = [dict(safety_ratio_obs=INF, replan=-1, agent=-1, obstacle=-1, sample=-1, below_one=0, compared=0) for _ in range(K)]
    agents = [dict(safety_ratio_obs=INF, replan=-1, obstacle=-1, sample=-1, reserved=0) for _ in range(n)]
    return missions, agents


def accumulate(missions, agents, offsets, safety_obs, finished, replans):
    """One replan, in place.  safety_obs: per global agent (safety_ratio_obs, closest_obstacle, sample); finished / replans: per mission,
    the record's words BEFORE this replan."""
    for k in range(len(offsets) - 1):
        if finished[k]:
            continue
        r = int(replans[k])
        least = (INF, -1, -1, -1)
        for a in range(int(offsets[k]), int(offsets[k + 1])):
            v, obstacle, sample = float(safety_obs[a][0]), int(safety_obs[a][1]), int(safety_obs[a][2])
            e = agents[a]
            if v < e["safety_ratio_obs"]:
                e.update(safety_ratio_obs=v, replan=r, obstacle=obstacle, sample=sample)
            if math.isfinite(v):
                missions[k]["compared"] += 1
            if v < 1.0:
                missions[k]["below_one"] += 1
            if v < least[0]:
                least = (v, a, obstacle, sample)
        m = missions[k]
        if least[0] < m["safety_ratio_obs"]:
            m.update(safety_ratio_obs=least[0], replan=r, agent=least[1], obstacle=least[2], sample=least[3])


def flight(offsets, steps):
    """A whole flight from the cleared state.  steps: per replan (safety_obs, finished, replans).  Returns (missions, agents)."""
    missions, agents = cleared(offsets)
    for safety_obs, finished, replans in steps:
        accumulate(missions, agents, offsets, safety_obs, finished, replans)
    return missions, agents


def as_arrays(np, mission_dtype, agent_dtype, missions, agents):
    """The two lists as numpy struct arrays of the given dtypes (api.MISSION_OBSTACLE_RECORD_DTYPE, api.AGENT_OBSTACLE_RECORD_DTYPE)."""
    ms, ag = np.zeros(len(missions), mission_dtype), np.zeros(len(agents), agent_dtype)
    for out, rows in ((ms, missions), (ag, agents)):
        for i, row in enumerate(rows):
            for f, v in row.items():
                out[f][i] = v
    return ms, ag
