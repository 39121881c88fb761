"""The work orders (include/lscqp.h: lscqp_order_by_work_device, lscqp_order_by_cost_device) at the sizes and key patterns where a counting
sort over 16 wavefronts with ballot peeling can go wrong: one element, sizes around a tile of 64 and around the workgroup of 1024, a
tile with 64 distinct keys, one key everywhere, the clamps of the iteration key, and costs at the edges of the 16 levels.  The order
decides which workgroup takes which instance, so anything but the expected permutation is an error: == throughout.  The order buffer
holds a sentinel first and carries a guard behind n, which must come back untouched."""
import numpy as np
import pytest

SIZES = [1, 2, 63, 64, 65, 1023, 1024, 1025, 1087, 4097]
SENTINEL, GUARD = -7, 256


def _in_tile_shuffle(g, keys):
    out = keys.copy()
    for lo in range(0, len(out), 64):
        g.shuffle(out[lo:lo + 64])
    return out


def iteration_patterns(n):
    g = np.random.default_rng(100 + n)
    i = np.arange(n)
    ordinary = g.integers(0, 64, n)
    clamped = ordinary.copy()
    clamped[g.permutation(n)[:max(1, n // 3)]] = g.choice([-3, 64, 1000], max(1, n // 3))  # below 0, just above 63, far above
    if n >= 3:
        clamped[[0, n // 2, n - 1]] = [1000, -3, 64]
    return {"all equal": np.full(n, 7), "all zero": np.zeros(n, int), "i % 64": i % 64, "i % 64 shuffled in its tile": _in_tile_shuffle(g, i % 64),
            "ascending": i * 63 // max(n - 1, 1), "descending": (n - 1 - i) * 63 // max(n - 1, 1), "-3, 64 and 1000 among ordinary ones": clamped,
            "random": ordinary}


def cost_patterns(n):
    g = np.random.default_rng(200 + n)
    i = np.arange(n, dtype=np.uint64)
    one = np.zeros(n, np.uint64)
    one[n // 2] = 9
    top32 = g.integers(0, 2 ** 32, n, dtype=np.uint64)
    top32[g.integers(0, n)] = 2 ** 32 - 1
    k = 1000  # top = 15 k: level j begins at cost j k
    edges = np.concatenate([np.arange(16) * k, np.arange(1, 16) * k - 1]).astype(np.uint64)
    at_edges = edges[g.integers(0, len(edges), n)]
    at_edges[: min(n, len(edges))] = np.sort(edges)[::-1][: min(n, len(edges))]  # (the top, 15 k, first: present at every n)
    return {"all equal": np.full(n, 5, np.uint64), "all zero": np.zeros(n, np.uint64), "one non-zero": one, "i % 64": i % 64,
            "i % 64 shuffled in its tile": _in_tile_shuffle(g, i % 64), "ascending": i, "descending": i[::-1].copy(), "top 2^32 - 1": top32,
            "all 2^32 - 1": np.full(n, 2 ** 32 - 1, np.uint64), "on the level boundaries of top 15000 and one below": at_edges,
            "random": g.integers(0, 100000, n, dtype=np.uint64)}


def _run(torch, n, launch, want, what):
    d_order = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    launch(d_order)
    torch.cuda.synchronize()
    order = d_order.cpu().numpy()
    assert (order[n:] == SENTINEL).all(), (what, "guard")
    assert np.array_equal(order[:n], want.astype(np.int32)), (what, order[:n][:80], want[:80])


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_order_by_work_is_the_stable_sort_of_the_clamped_iterations(api, torch_cuda, n):
    torch = torch_cuda
    for name, it in iteration_patterns(n).items():
        info = np.zeros(n, api.INFO_DTYPE)
        info["iterations"] = it
        info["flags"], info["gap"] = -1, np.nan  # (nothing but the iterations is read)
        d_info = torch.from_numpy(info.view(np.uint8).reshape(-1).copy()).cuda()
        want = np.argsort(63 - np.clip(np.asarray(it, dtype=np.int64), 0, 63), kind="stable")
        _run(torch, n, lambda d_order: api.Solver.order_by_work_device(n, d_info, d_order), want, (n, name))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_order_by_cost_is_the_stable_sort_of_the_sixteen_levels(api, torch_cuda, n):
    torch = torch_cuda
    for name, cost in cost_patterns(n).items():
        c = np.asarray(cost, dtype=np.int64)
        assert c.min() >= 0 and c.max() < 2 ** 32
        d_cost = torch.from_numpy(c.astype(np.uint32).view(np.int32).copy()).cuda()
        want = np.argsort(15 - (c * 15) // max(int(c.max()), 1), kind="stable")
        _run(torch, n, lambda d_order: api.Solver.order_by_cost_device(n, d_cost, d_order), want, (n, name))


def test_the_patterns_hold_what_they_are_there_for():
    """Every full tile of the `i % 64` patterns has 64 distinct keys; the clamp pattern
    has all three out-of-range values; the boundary pattern has all sixteen level starts and the cost below each."""
    for n in SIZES:
        it, co = iteration_patterns(n), cost_patterns(n)
        for name in ("i % 64", "i % 64 shuffled in its tile"):
            for lo in range(0, n - 63, 64):
                assert len(set(it[name][lo:lo + 64].tolist())) == 64 and len(set(co[name][lo:lo + 64].tolist())) == 64
        if n >= 3:
            assert {-3, 64, 1000} <= set(it["-3, 64 and 1000 among ordinary ones"].tolist())
        edges = co["on the level boundaries of top 15000 and one below"]
        assert edges.max() == 15000
        if n >= 63:
            assert set(edges.tolist()) >= set(range(0, 15001, 1000)) | set(range(999, 15000, 1000))
