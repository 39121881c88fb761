"""lscqp_obstacles_drive_device alone (csrc/lscobstacle.hip: obstacle_drive_kernel), followed by lscqp_obstacles_advance_device as in the
chain, against the numpy restatement (tests/obstacle_drive_reference.py): every byte of the table after every replan.  Bit for bit: the
kernel uses + - x / sqrt only, in the restatement's order, without contraction.  The scenario is tests/obstacle_drive_cases.py's (the CPU
test shows that it takes every branch both ways); the expected tables are computed once per variant and left unchanged."""
import numpy as np
import pytest

from tests import obstacle_drive_cases as Cs
from tests import obstacle_drive_reference as D

pytestmark = pytest.mark.gpu


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


class Device:
    """One table on the device with everything the two kernels read; `replan` runs (drive, advance) at the clock's value and downloads."""

    def __init__(self, api, torch, sol, sc, time_step, state_at=Cs.state_at):
        self.api, self.torch, self.sol, self.sc, self.time_step, self.state_at = api, torch, sol, sc, time_step, state_at
        self.n = len(sc["models"])
        self.models, self.drives = _dev(torch, sc["models"]), _dev(torch, sc["drives"])
        self.history = _dev(torch, sc["history"]) if len(sc["history"]) else None
        self.table = _dev(torch, sc["table0"])
        self.ckpt = torch.zeros(self.n * api.OBSTACLE_DRIVE_STATE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        self.clock = torch.zeros(1, dtype=torch.int32, device="cuda")

    def replan(self, r=None):
        torch = self.torch
        if r is not None:
            self.clock.fill_(r)
        r = int(self.clock.cpu()[0])
        st = self.state_at(r)
        state = _dev(torch, st)
        self.sol.obstacles_drive_device(self.models, self.drives, self.n, self.history, len(self.sc["history"]), state, len(st), self.ckpt, self.time_step,
                                        self.clock, self.table)
        self.sol.obstacles_advance_device(self.models, self.n, self.time_step, self.clock, self.table)
        torch.cuda.synchronize()
        assert int(self.clock.cpu()[0]) == r + 1  # (the drive reads the clock, the advance counts it)
        return np.frombuffer(self.table.cpu().numpy().tobytes(), self.api.OBSTACLE_DTYPE)

    def checkpoints(self):
        return np.frombuffer(self.ckpt.cpu().numpy().tobytes(), self.api.OBSTACLE_DRIVE_STATE_DTYPE)


@pytest.fixture(scope="module")
def sol(api, torch_cuda):
    s = api.Solver(api.make_desc(M=5, dim=3))
    yield s
    s.close()


@pytest.mark.parametrize("twins, time_step", [(False, 0.2), (False, 0.15), (True, 0.2)], ids=["step_0.2", "step_0.15", "twins"])
def test_every_table_byte_is_the_restatements_over_forty_replans(api, torch_cuda, sol, twins, time_step):
    sc = Cs.scenario(api, twins)
    want, _ = Cs.reference_flight(sc, time_step)
    dev = Device(api, torch_cuda, sol, sc, time_step)
    for r in range(Cs.K):
        got = dev.replan()
        assert got.tobytes() == want[r].tobytes(), (r, [i for i in range(6) if got[i].tobytes() != want[r][i].tobytes()])
    assert np.abs(want[-1]["position"][Cs.CHASER_A] - want[0]["position"][Cs.CHASER_A]).max() > 0.1
    assert want[-1][Cs.HELD].tobytes() == sc["table0"][Cs.HELD].tobytes()


def chasers(api, n):
    """n chasers of one another on a jittered lattice of 0.5 m pitch (radius 0.2: the neighbours are inside Q* = 0.8), each flying to a goal
    of its own: every thread reads every other entry, and with n > 64 a thread writes entries while others still read."""
    rng = np.random.default_rng(n)
    side = int(np.ceil(n ** (1 / 3)))
    cell = np.array([(i, j, k) for i in range(side) for j in range(side) for k in range(side)][:n], np.float64)
    start = 0.5 * cell + rng.uniform(-0.05, 0.05, (n, 3))
    specs = [dict(type="chasing", start=start[i].tolist(), size=0.2, max_vel=0.8, max_acc=2.0, gamma_target=0.7, gamma_obs=1.5, downwash=1.0,
                  goal=rng.uniform(-1, 4, 3).tolist()) for i in range(n)]
    models = api.obstacle_model_prepare(api.obstacle_models(specs))
    drives, history = api.obstacle_drives(specs, 0)
    return dict(models=models, drives=drives, history=history, table0=_reset(api, models))


def _reset(api, models):
    t = np.zeros(len(models), api.OBSTACLE_DTYPE)
    t["position"] = np.float32(models["start"])
    t["radius"], t["downwash"], t["max_acc"] = models["radius"], models["downwash"], models["max_acc"]
    return t


@pytest.mark.parametrize("size, replans", [(1, 10), (2, 10), ("max", 3)])
def test_tables_of_chasers_of_one_another(api, torch_cuda, sol, size, replans):
    n = sol.max_obstacles() if size == "max" else size
    assert size != "max" or n > 64  # (more obstacles than threads: the strided loop)
    sc = chasers(api, n)
    dev = Device(api, torch_cuda, sol, sc, 0.2, state_at=lambda r: np.zeros((0, 9)))
    table = sc["table0"].copy()
    D.counts.clear()
    for r in range(replans):
        D.drive_table(sc["models"], sc["drives"], sc["history"], table, None, r, 0.2)
        got = dev.replan()
        assert got.tobytes() == table.tobytes(), (r, [i for i in range(n) if got[i].tobytes() != table[i].tobytes()][:8])
    assert np.abs(table["position"] - sc["table0"]["position"]).max() > 0.01
    assert n == 1 or D.counts["repulsion_inside"] > 0


def test_a_clock_written_back_from_10_to_3_gives_the_from_zero_value(api, torch_cuda, sol):
    sc = Cs.scenario(api)
    replans = list(range(10)) + [3, 4]
    want, _ = Cs.reference_flight(sc, 0.2, replans)
    dev = Device(api, torch_cuda, sol, sc, 0.2)
    for k, r in enumerate(replans):
        got = dev.replan(r)
        assert got.tobytes() == want[k].tobytes(), (k, r)
        if r == 9:
            assert dev.checkpoints()["i_done"][Cs.GAUSS] == 18
    assert dev.checkpoints()["i_done"][Cs.GAUSS] == 8
    # the gaussian obstacle at clock 3 is the loop from zero at t = 0.6, whatever came before
    g = D.Gaussian(sc["models"]["start"][Cs.GAUSS], sc["drives"]["initial_vel"][Cs.GAUSS], sc["drives"]["max_vel"][Cs.GAUSS], 0.1, sc["history"])
    p, v, _ = g.at(D.R.clock_time(3, 0.2))
    assert (want[10]["position"][Cs.GAUSS] == np.float64(p)).all() and (want[10]["velocity"][Cs.GAUSS] == np.float64(v)).all()


def test_a_clock_that_jumps_forward_by_fifty(api, torch_cuda, sol):
    sc = Cs.scenario(api)
    replans = [0, 1, 2, 52, 53]
    want, _ = Cs.reference_flight(sc, 0.2, replans)
    dev = Device(api, torch_cuda, sol, sc, 0.2)
    for k, r in enumerate(replans):
        got = dev.replan(r)
        assert got.tobytes() == want[k].tobytes(), (k, r)
    assert dev.checkpoints()["i_done"][Cs.GAUSS] == 106 and want[-1]["reserved"][Cs.GAUSS] == D.HISTORY_ENDED
