"""Neighbour selection at ties, on the device: lscqp_select_neighbours_device and lscqp_select_neighbours_missions_device on every constructed
pack of tests/neighbour_cases.py, held to the rule in numpy with ==.  The list and count buffers hold a sentinel first and carry a guard
region behind them, which must come back untouched.  One launch per pack and window."""
import numpy as np
import pytest

from tests import neighbour_cases as NC

pytestmark = pytest.mark.gpu
SENTINEL, GUARD = -7, 256


@pytest.fixture(scope="module")
def solver(api, torch_cuda):
    sol = api.Solver(api.make_desc(M=5, dim=3))
    yield sol
    sol.close()


def _buffers(torch, n_agents, n_obs):
    d_nbr = torch.full((n_agents * n_obs + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    d_cnt = torch.full((n_agents + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    return d_nbr, d_cnt


def _held_to(d_nbr, d_cnt, n_agents, n_obs, want_nbr, want_cnt, what):
    nbr, cnt = d_nbr.cpu().numpy(), d_cnt.cpu().numpy()
    assert (nbr[n_agents * n_obs:] == SENTINEL).all() and (cnt[n_agents:] == SENTINEL).all(), what  # the guards
    assert np.array_equal(cnt[:n_agents], want_cnt), what
    got = nbr[:n_agents * n_obs].reshape(n_agents, n_obs)
    bad = np.flatnonzero((got != want_nbr).any(axis=1))
    assert bad.size == 0, (what, "first wrong row", int(bad[0]), got[bad[0]].tolist(), want_nbr[bad[0]].tolist())


@pytest.mark.parametrize("pack", NC.PACKS, ids=repr)
def test_single_entry_follows_the_rule(solver, torch_cuda, pack):
    """The launched window of the pack; a pack with a partition runs each mission as a swarm of its own, ids shifted back."""
    torch = torch_cuda
    if pack.offsets is None:
        runs = [(pack.pos, pack.first, pack.n_agents, 0, pack.ref())]
    else:
        r, off = pack.ref(), pack.offsets
        runs = [(pack.pos[lo:hi], 0, hi - lo, lo, NC.Ref(r.nbr[lo:hi], r.cnt[lo:hi], None, None)) for lo, hi in zip(off[:-1], off[1:])]
    for pos, first, n_agents, shift, want in runs:
        d_nbr, d_cnt = _buffers(torch, n_agents, pack.n_obs)
        solver.select_neighbours_device(n_agents, first, len(pos), pack.n_obs, pack.rng, torch.from_numpy(np.ascontiguousarray(pos)).cuda(),
                                        d_nbr if pack.n_obs else None, d_cnt)
        torch.cuda.synchronize()
        _held_to(d_nbr, d_cnt, n_agents, pack.n_obs, np.where(want.nbr >= 0, want.nbr - shift, want.nbr), want.cnt, (pack, shift))


@pytest.mark.parametrize("pack", NC.PACKS, ids=repr)
def test_missions_entry_follows_the_rule(solver, torch_cuda, pack):
    """Every agent of the pack (the entry has no window); a pack without a partition is one mission."""
    torch = torch_cuda
    off = [0, pack.n] if pack.offsets is None else pack.offsets
    want = pack.ref(whole=True)
    d_nbr, d_cnt = _buffers(torch, pack.n, pack.n_obs)
    solver.select_neighbours_missions_device(off, pack.n_obs, pack.rng, torch.from_numpy(pack.pos).cuda(), d_nbr if pack.n_obs else None, d_cnt)
    torch.cuda.synchronize()
    _held_to(d_nbr, d_cnt, pack.n, pack.n_obs, want.nbr, want.cnt, pack)
