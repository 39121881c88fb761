"""lscqp_obstacles_advance_device alone (csrc/lscobstacle.hip: obstacle_advance_kernel) against the numpy restatement of the reference's
models (tests/obstacle_reference.py): one table of all four kinds mixed, advanced clock value by clock value through every phase
boundary of its straight obstacles and into the third lap of its patrols.

What is compared how, and why:
  straight obstacles, patrols in their first lap   bit for bit: the same float32 / double operations in the same order
  patrols in later laps, spins                     within one float32 ulp of the coordinate: the kernel takes whole laps off the time in
                                                   one step where the reference subtracts leg by leg, and its sin / cos are the device's;
                                                   both move the double result by a few ulps (~1e-13 m), which can flip one float32 rounding
  velocities of those                              within one float32 ulp of `speed`
The straight obstacles are placed so that their boundaries t1, t2, t3 are multiples of the time step (up to the rounding of either
side), so the clock values hit them, and the values one step before and after are flown too: the phase a boundary value falls in is
part of the bit-for-bit claim."""
import numpy as np
import pytest

from tests import obstacle_reference as R

pytestmark = pytest.mark.gpu

TIME_STEP = 0.2
STEPS = 60          # clock values 0 .. 59: 11.8 s
SENTINEL = 0xA5
TAIL = 3            # table entries behind n_dyn


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _specs(n):
    """n mission-file entries.  The first ones are the constructed cases, the rest random ones of every kind in turn."""
    S = [
        # long branch, t1 = 0.4, t2 = 2.0, t3 = 2.4 (speed / max_acc = 0.4, dist_acc = 0.2, dist = 2): along x, and along a diagonal of length 3
        # (t2 = 3.0, t3 = 3.4)
        dict(type="straight", start=[-1, 0.5, 1], goal=[1, 0.5, 1], size=0.2, speed=1.0, max_acc=2.5, downwash=1.0),
        dict(type="straight", start=[0, 0, 0], goal=[1, 2, 2], size=0.3, speed=1.0, max_acc=2.5, downwash=2.0),
        # short branch: dist_acc = 2, dist = 2: t1 = 1.0, t2 = 2.0; dist_acc = 0.78125, dist = 0.5: t1 = 0.8, t2 = 1.6
        dict(type="straight", start=[0, -1, 1], goal=[0, 1, 1], size=0.2, speed=2.0, max_acc=1.0, downwash=1.0),
        dict(type="straight", start=[0.25, 0, 1], goal=[0.25, 0, 1.5], size=0.2, speed=1.25, max_acc=1.0, downwash=1.0),
        # patrols of 2, 3 and 8 waypoints whose third lap starts inside the flight: legs of 0.55 s (dist 0.3, speed 1, max_acc 4)
        dict(type="patrol", waypoints=[[0, 0, 1], [0.3, 0, 1]], size=0.2, speed=1.0, max_acc=4.0, downwash=1.0),
        dict(type="patrol", waypoints=[[0, 0, 1], [0.3, 0, 1], [0.3, 0.3, 1]], size=0.2, speed=1.0, max_acc=4.0, downwash=1.0),
        dict(type="patrol", waypoints=[[0.3 * np.cos(k * np.pi / 4) / (2 * np.sin(np.pi / 8)), 0.3 * np.sin(k * np.pi / 4) / (2 * np.sin(np.pi / 8)), 1 + 0.01 * k]
                                       for k in range(8)], size=0.2, speed=1.0, max_acc=4.0, downwash=1.0),
        dict(type="spin", axis=[0, 0, 1, 0, 0, 1], start=[1.5, 0, 1], size=0.2, speed=1.0, max_acc=2.0, downwash=1.0),
        dict(type="chasing", start=[9, 9, 9], size=0.2, max_acc=1.0, downwash=1.0),
    ]
    rng = np.random.default_rng(11)
    while len(S) < n:
        k = len(S) % 5
        if k == 0:    # long or short, as it falls
            S.append(dict(type="straight", start=rng.uniform(-3, 3, 3).tolist(), goal=rng.uniform(-3, 3, 3).tolist(), size=0.2,
                          speed=float(rng.uniform(0.3, 1.5)), max_acc=float(rng.uniform(0.5, 3.0)), downwash=1.0))
        elif k == 1:  # short: a hop of a few centimetres
            s0 = rng.uniform(-3, 3, 3)
            S.append(dict(type="straight", start=s0.tolist(), goal=(s0 + rng.uniform(-0.2, 0.2, 3)).tolist(), size=0.2,
                          speed=float(rng.uniform(1.0, 2.0)), max_acc=float(rng.uniform(0.5, 1.5)), downwash=1.0))
        elif k == 2:  # a patrol of 2 .. 8 waypoints within a metre: laps of a few seconds
            c = rng.uniform(-3, 3, 3)
            S.append(dict(type="patrol", waypoints=(c + rng.uniform(-0.5, 0.5, (int(rng.integers(2, 9)), 3))).tolist(), size=0.25,
                          speed=float(rng.uniform(1.0, 2.0)), max_acc=float(rng.uniform(2.0, 5.0)), downwash=1.5))
        elif k == 3:
            S.append(dict(type="spin", axis=np.concatenate([rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)]).tolist(), start=rng.uniform(1.5, 3, 3).tolist(),
                          size=0.3, speed=float(rng.uniform(0.3, 1.5)), max_acc=3.0, downwash=1.0))
        else:
            S.append(dict(type="gaussian", start=rng.uniform(-3, 3, 3).tolist(), size=0.2, max_acc=1.0, downwash=1.0))
    return S[:n]


@pytest.fixture(scope="module")
def world(api):
    """The largest table, prepared, and the restatement's positions / velocities of all its models at every clock value: computed once,
    shared by every size (a smaller table is the first n models of this one) and left unchanged."""
    sol = api.Solver(api.make_desc(M=5, dim=3))
    n_max = sol.max_obstacles()
    raw = api.obstacle_models(_specs(n_max))
    models = api.obstacle_model_prepare(raw)
    objs = [R.from_model(m) for m in raw]
    pos, vel = np.full((STEPS, n_max, 3), np.nan, np.float32), np.full((STEPS, n_max, 3), np.nan, np.float32)
    for r in range(STEPS):
        t = R.clock_time(r, TIME_STEP)
        for i, o in enumerate(objs):
            if o is not None:
                pos[r, i], vel[r, i] = o.at(t)
    pos.setflags(write=False), vel.setflags(write=False)
    yield dict(sol=sol, n_max=n_max, raw=raw, models=models, objs=objs, pos=pos, vel=vel)
    sol.close()


def _fly(torch, api, W, n, steps):
    """The first n models advanced `steps` times from clock 0: tables [steps] (n + TAIL entries, as bytes went) and the clock values read."""
    d_models = _dev(torch, W["models"][:n])
    d_table = torch.full(((n + TAIL) * api.OBSTACLE_DTYPE.itemsize,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_clock = torch.zeros(1, dtype=torch.int32, device="cuda")
    tables, clocks = [], []
    for _ in range(steps):
        W["sol"].obstacles_advance_device(d_models, n, TIME_STEP, d_clock, d_table)
        torch.cuda.synchronize()
        tables.append(d_table.cpu().numpy().copy())
        clocks.append(int(d_clock.cpu()[0]))
    return tables, clocks


def ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def test_the_constructed_cases_are_what_they_are_meant_to_be(world):
    o = world["objs"]
    near = lambda a, b: abs(a - b) < 1e-6  # noqa: E731
    assert all(near(a, b) for a, b in zip(o[0].phases(), (0.4, 2.0, 2.4))) and all(near(a, b) for a, b in zip(o[1].phases(), (0.4, 3.0, 3.4)))
    assert all(near(a, b) for a, b in zip(o[2].phases(), (1.0, 2.0))) and all(near(a, b) for a, b in zip(o[3].phases(), (0.8, 1.6)))
    end = R.clock_time(STEPS - 1, TIME_STEP)
    for i, nw in ((4, 2), (5, 3), (6, 8)):
        assert len(o[i].legs) == nw and 2 * o[i].lap_time() < end, (i, o[i].lap_time())  # the flight reaches the third lap
    kinds = world["models"]["kind"]
    assert all((kinds[:65] == k).sum() >= 5 for k in range(4)) and (kinds == 0).sum() > 40


@pytest.mark.parametrize("n", [1, 63, 64, 65, "max"])
def test_the_table_equals_the_restatement_at_every_clock_value(api, torch_cuda, world, n):
    torch, W = torch_cuda, world
    n = W["n_max"] if n == "max" else n
    tables, clocks = _fly(torch, api, W, n, STEPS)
    assert clocks == list(range(1, STEPS + 1))
    m, objs = W["models"][:n], W["objs"][:n]
    held = m["kind"] == api.OBSTACLE_HELD
    exact = np.array([isinstance(o, R.Straight) for o in objs])
    patrol = np.array([isinstance(o, R.Patrol) for o in objs])
    lap = np.array([o.lap_time() if isinstance(o, R.Patrol) else np.inf for o in objs])
    isz = api.OBSTACLE_DTYPE.itemsize
    seen_later_lap = 0
    for r, raw in enumerate(tables):
        T = raw[:n * isz].view(api.OBSTACLE_DTYPE)
        # HELD entries and everything behind n_dyn: untouched
        assert (raw[n * isz:] == SENTINEL).all(), r
        assert (T[held].view(np.uint8) == SENTINEL).all(), r
        live = ~held
        for f in ("radius", "downwash", "max_acc"):
            assert np.array_equal(T[f][live], m[f][live]), (r, f)
        assert (T["type"][live] == 0).all() and (T["reserved"][live] == 0).all()
        pos, vel = T["position"], T["velocity"]
        # float32 values held in double
        assert np.array_equal(pos[live], pos[live].astype(np.float32).astype(np.float64)) and np.array_equal(vel[live], vel[live].astype(np.float32).astype(np.float64))
        want_p, want_v = W["pos"][r, :n].astype(np.float64), W["vel"][r, :n].astype(np.float64)
        first_lap = patrol & (R.clock_time(r, TIME_STEP) < lap)
        bit = exact | first_lap
        assert np.array_equal(pos[bit], want_p[bit]), (r, np.nonzero(bit & (pos != want_p).any(1))[0])
        assert np.array_equal(vel[bit], want_v[bit]), (r, np.nonzero(bit & (vel != want_v).any(1))[0])
        rest = live & ~bit
        seen_later_lap += int((patrol & rest).sum())
        if rest.any():
            dp = np.abs(pos[rest] - want_p[rest])
            tol = np.maximum(ulp32(pos[rest]), ulp32(want_p[rest]))
            assert (dp <= tol).all(), (r, np.nonzero(rest)[0][(dp > tol).any(1)], dp.max())
            dv = np.abs(vel[rest] - want_v[rest])
            assert (dv <= ulp32(m["speed"][rest])[:, None]).all(), (r, np.nonzero(rest)[0][(dv > ulp32(m["speed"][rest])[:, None]).any(1)], dv.max())
    if n >= 7:
        assert seen_later_lap > 0


def test_twenty_flights_from_a_reset_clock_are_bit_identical(api, torch_cuda, world):
    first = None
    for _ in range(20):
        tables, clocks = _fly(torch_cuda, api, world, 65, 12)
        got = np.concatenate(tables).tobytes()
        first = got if first is None else first
        assert got == first and clocks == list(range(1, 13))


def test_the_clock_is_the_callers_word(api, torch_cuda, world):
    """The kernel evaluates the replan the word names and stores that + 1: a caller that writes 37 gets replan 37."""
    torch, W = torch_cuda, world
    n = 9
    d_models = _dev(torch, W["models"][:n])
    d_table = torch.zeros(n * api.OBSTACLE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_clock = torch.full((1,), 37, dtype=torch.int32, device="cuda")
    W["sol"].obstacles_advance_device(d_models, n, TIME_STEP, d_clock, d_table)
    torch.cuda.synchronize()
    T = d_table.cpu().numpy().view(api.OBSTACLE_DTYPE)
    assert int(d_clock.cpu()[0]) == 38
    for i in range(4):  # the straight ones: bit for bit
        assert np.array_equal(T["position"][i], W["pos"][37, i].astype(np.float64)) and np.array_equal(T["velocity"][i], W["vel"][37, i].astype(np.float64))
