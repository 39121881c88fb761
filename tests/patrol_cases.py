"""Inputs shared by tests/test_patrol_cpu.py (lscqp_patrol_host against the restatement, no device) and tests/test_patrol_gpu.py (the kernel
against the restatement): a constructed table that takes the PATROL branch both ways at its edges, a scripted back-and-forth, and seeded
batches for the kernel's sizes.  Every case is a CALL: n agents, one threshold."""
import numpy as np

from tests import patrol_reference as PR

f32 = np.float32
Z = 1.0


def _call(name, pos, desired, start, threshold, dim=2, z_2d=Z, expect=None, calls=1, legs=None):
    pos, desired, start = (np.array(v, np.float64).reshape(-1, 3) for v in (pos, desired, start))
    state = np.zeros((len(pos), 9))
    state[:, :3] = pos
    state[:, 3:] = 0.25  # (velocities and accelerations are nobody's business here)
    return dict(name=name, state=state, desired=desired, start=start, threshold=float(threshold), dim=dim, z_2d=float(z_2d),
                expect=None if expect is None else np.array(expect, np.int32).reshape(-1), calls=calls,
                legs=None if legs is None else np.array(legs, np.int32).reshape(-1))


def table():
    """The constructed calls.  expect: swapped after the LAST call; legs: legs after the last call (None: expect, for one call)."""
    up32 = lambda v: float(np.nextafter(f32(v), f32(np.inf)))   # noqa: E731  (one float32 ulp above (float)v, as a double)
    dn32 = lambda v: float(np.nextafter(f32(v), f32(-np.inf)))  # noqa: E731
    D11 = PR.distance([1.1, 0, Z], [0, 0, Z])
    T = [
        # exactly at the threshold: 0.5 < 0.5 is false (the record's `>` calls the same mission finished)
        _call("at_threshold", [0, 0, Z], [0.5, 0, Z], [9, 9, Z], 0.5, expect=[0]),
        _call("just_above_threshold", [0, 0, Z], [0.5, 0, Z], [9, 9, Z], np.nextafter(0.5, 1.0), expect=[1]),
        # a goal that float32 does not hold: (float)1.1 = 1.10000002384 > 1.1, (float)0.9 = 0.89999997616 < 0.9.  In double arithmetic the
        # first would turn at 1.1000000001 and the second would not at 0.9
        _call("f32_goal_above_its_double", [0, 0, Z], [1.1, 0, Z], [9, 9, Z], 1.1000000001, expect=[0]),
        _call("f32_goal_below_its_double", [0, 0, Z], [0.9, 0, Z], [9, 9, Z], 0.9, expect=[1]),
        # ... and one float32 ulp either side of it, at the threshold that is the restatement's distance to (float)1.1 itself (the square is
        # rounded to float32 too, so that distance is not (float)1.1; neighbouring floats near 1.1 have distinct squares)
        _call("f32_goal_at_itself", [0, 0, Z], [1.1, 0, Z], [9, 9, Z], D11, expect=[0]),
        _call("f32_goal_one_ulp_further", [0, 0, Z], [up32(1.1), 0, Z], [9, 9, Z], D11, expect=[0]),
        _call("f32_goal_one_ulp_nearer", [0, 0, Z], [dn32(1.1), 0, Z], [9, 9, Z], D11, expect=[1]),
        # a 2-D agent flies in its plane whatever the state's third word holds
        _call("plane_wins_and_turns", [0, 0, 5.0], [0.3, 0, Z], [9, 9, Z], 0.5, expect=[1]),
        _call("plane_wins_and_stays", [0, 0, Z], [0.3, 0, Z], [9, 9, Z], 0.5, z_2d=5.0, expect=[0]),
        # 3-D: the state's own z
        _call("three_d_far_in_z", [1, 2, 3], [1.3, 2.4, 5.0], [9, 9, 9], 0.6, dim=3, expect=[0]),
        _call("three_d_near", [1, 2, 3], [1.3, 2.4, 3.0], [9, 9, 9], 0.6, dim=3, expect=[1]),
        _call("three_d_z_alone", [1, 2, 3], [1, 2, 3.5], [9, 9, 9], 0.5, dim=3, expect=[0]),
        # start and goal both within the threshold: turns in two consecutive calls and is back where it began
        _call("there_and_back", [0.1, 0, Z], [0.2, 0, Z], [0, 0, Z], 0.5, expect=[1], calls=2, legs=[2]),
        # threshold 0: no distance is below it, not even 0
        _call("threshold_zero_on_the_goal", [0.5, 0.5, Z], [0.5, 0.5, Z], [9, 9, Z], 0.0, expect=[0]),
        # a mixed call: agents either side in one launch
        _call("mixed", [[0, 0, Z], [0, 0, Z], [2, 2, Z]], [[0.5, 0, Z], [0.25, 0.25, Z], [2, 2, Z]], [[1, 1, Z], [2, 2, Z], [3, 3, Z]], 0.5,
              expect=[0, 1, 1]),
    ]
    # seeded pairs whose threshold is the restatement's own distance (does not turn) and the next double above it (turns)
    rnd = np.random.default_rng(32)
    for i in range(12):
        dim = 2 + (i & 1)
        pos, goal = rnd.uniform(-3, 3, 3), rnd.uniform(-3, 3, 3)
        d = PR.distance(goal, PR.position_of(pos, dim, Z))
        T.append(_call("seeded_%d_at" % i, pos, goal, [9, 9, 9], d, dim=dim, expect=[0]))
        T.append(_call("seeded_%d_above" % i, pos, goal, [9, 9, 9], np.nextafter(d, np.inf), dim=dim, expect=[1]))
    return T


def batch(n, seed, threshold=0.5, dim=2):
    """n agents scattered around their goals so that about half of them are within the threshold; some exactly on it."""
    rnd = np.random.default_rng(seed)
    goal = rnd.uniform(-5, 5, (n, 3))
    start = rnd.uniform(-5, 5, (n, 3))
    r = rnd.uniform(0.0, 2 * threshold, n)
    th = rnd.uniform(0, 2 * np.pi, n)
    pos = goal + np.c_[r * np.cos(th), r * np.sin(th), np.zeros(n)]
    if dim == 2:
        goal[:, 2] = Z
        pos[:, 2] = rnd.uniform(-1, 1, n)  # (ignored: the plane wins)
    pos[::7] = goal[::7] + np.array([threshold, 0, 0])  # on the threshold up to the rounding of the sum
    start[1::3] = pos[1::3] + np.array([0.1 * threshold, 0, 0])  # a third start next to where they are: whoever turns, turns back in the next call
    if dim == 2:
        start[1::3, 2] = Z
    return _call("batch_%d" % n, pos, goal, start, threshold, dim=dim)


def scripted_flight(step, calls=40, n=5, speed=0.3, threshold=0.1):
    """n agents on legs of different lengths fly towards their desired goal at `speed` per call and stop on it; `step(case)` runs ONE
    transition in place on the case's arrays (state, desired, start, legs, swapped).  Returns the per-call (desired, start, legs, swapped)."""
    start = np.array([[0.0, 0.1 * a, Z] for a in range(n)])
    goal = np.array([[0.7 + 0.45 * a, 0.1 * a, Z] for a in range(n)])
    c = _call("flight", start.copy(), goal.copy(), start.copy(), threshold)
    c["legs"], c["swapped"] = np.zeros(n, np.int32), np.full(n, -1, np.int32)
    out = []
    for _ in range(calls):
        step(c)
        out.append((c["desired"].copy(), c["start"].copy(), c["legs"].copy(), c["swapped"].copy()))
        to = c["desired"] - c["state"][:, :3]
        d = np.sqrt((to * to).sum(1))
        move = np.where(d > speed, speed / np.maximum(d, 1e-300), 1.0)
        c["state"][:, :3] = np.float32(c["state"][:, :3] + to * move[:, None]).astype(np.float64)
    return out
