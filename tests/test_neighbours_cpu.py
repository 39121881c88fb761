"""Neighbour selection at ties, on the CPU: the oracle's orc_select_neighbours against the rule in numpy (tests/neighbour_cases.py) on
every constructed pack, and every pack's own statement -- which path it reaches, where its cut falls -- from the reference alone."""
import numpy as np
import pytest

from tests import neighbour_cases as NC


@pytest.mark.parametrize("pack", NC.PACKS, ids=repr)
def test_pack_is_what_it_says_and_the_oracle_follows_the_rule(oracle, pack):
    share = pack.check()
    r = pack.ref()
    print("%-36s %4d agents, window [%d, %d), n_obs %4d: in range %d..%d, cut inside a tie group for %3.0f %% of the window"
          % (pack.name, pack.n, pack.first, pack.first + pack.n_agents, pack.n_obs, r.cnt.min(), r.cnt.max(), 100 * share))
    if pack.offsets is None:
        nbr, cnt = oracle.select_neighbours(pack.pos, pack.n_obs, pack.rng, first=pack.first, n_agents=pack.n_agents)
        assert np.array_equal(cnt, r.cnt) and np.array_equal(nbr, r.nbr)
        return
    off = pack.offsets  # the oracle has no partition: each mission on its own, ids shifted
    for k in range(len(off) - 1):
        lo, hi = int(off[k]), int(off[k + 1])
        sel = slice(max(lo, hi - 12), hi) if hi - lo > 64 else slice(lo, hi)  # (the oracle drops one agent at a time: a window of the large one)
        nbr, cnt = oracle.select_neighbours(pack.pos[lo:hi], pack.n_obs, pack.rng, first=sel.start - lo, n_agents=sel.stop - sel.start)
        assert np.array_equal(cnt, r.cnt[sel]) and np.array_equal(np.where(nbr >= 0, nbr + lo, nbr), r.nbr[sel]), k


def test_the_lattice_of_a_real_start_is_cut_inside_a_tie_group_everywhere():
    """12 x 12 x 11 agents, spacing 0.5, n_obs = 8: the smallest first shell is a corner's 7, so the 8th and 9th nearest share a distance
    for every agent (a window of it here; the reference is the same for all)."""
    P = NC.lattice(12, 12, 11, 0.5)
    r = NC.reference(P, 8, 0.0, first=0, n_agents=160)  # includes corners, edges, faces and interior agents
    assert r.tie.all() and (r.cnt == len(P) - 1).all()


def test_reference_against_the_plain_loop():
    """The vectorised reference against the definition written out (tests/test_lscmode.py: _numpy_neighbours) on random positions with a
    coincident pair, with and without a partition."""
    from tests.test_lscmode import _numpy_neighbours

    rng = np.random.default_rng(5)
    P = np.float32(rng.uniform(-4, 4, (90, 3))).astype(np.float64)
    P[11] = P[4]
    for n_obs, r_ in ((6, 3.0), (100, 0.0), (1, 2.0)):
        ref = NC.reference(P, n_obs, r_, first=20, n_agents=50)
        for a in range(20, 70):
            want, c = _numpy_neighbours(P, a, n_obs, r_)
            assert ref.nbr[a - 20].tolist() == want and ref.cnt[a - 20] == c
        off = [0, 30, 31, 90]
        ref = NC.reference(P, n_obs, r_, offsets=off)
        for k in range(3):
            for a in range(off[k], off[k + 1]):
                want, c = _numpy_neighbours(P[off[k]:off[k + 1]], a - off[k], n_obs, r_)
                assert ref.nbr[a].tolist() == [j + off[k] if j >= 0 else j for j in want] and ref.cnt[a] == c
