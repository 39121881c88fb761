"""lscqp_patrol_device and lscqp_field_exchange_device alone (csrc/lscpatrol.hip: patrol_kernel, field_exchange_kernel) against the numpy
restatement (tests/patrol_reference.py) and against synthetic fields, byte for byte, with sentinels behind and guard words around every
buffer the kernels write."""
import numpy as np
import pytest

from tests import patrol_cases as Cs
from tests import patrol_reference as PR

pytestmark = pytest.mark.gpu
SENT_F, SENT_I, PAD = -12345.678, -77, 64
CHUNK = 1024  # field_exchange_kernel: words of a slice per workgroup


@pytest.fixture(scope="module")
def solver(api):
    sol = api.Solver(api.make_desc(M=5, dim=3))
    yield sol
    sol.close()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _device_call(torch, solver, c, calls=1):
    """The case on the device, every written buffer with PAD sentinel entries behind n -> (desired, start, legs, swapped) and the tails."""
    n = len(c["state"])
    d = np.full((n + PAD, 3), SENT_F)
    s = np.full((n + PAD, 3), SENT_F)
    d[:n], s[:n] = c["desired"], c["start"]
    legs, sw = np.full(n + PAD, SENT_I, np.int32), np.full(n + PAD, SENT_I, np.int32)
    legs[:n] = 0
    dd, ds, dl, dw, dst = _dev(torch, d), _dev(torch, s), _dev(torch, legs), _dev(torch, sw), _dev(torch, c["state"])
    for _ in range(calls):
        solver.patrol_device(n, dst, dd, ds, c["threshold"], c["dim"], c["z_2d"], dl, dw)
    torch.cuda.synchronize()
    out = [t.cpu().numpy() for t in (dd, ds, dl, dw)]
    assert (out[0][n:] == SENT_F).all() and (out[1][n:] == SENT_F).all() and (out[2][n:] == SENT_I).all() and (out[3][n:] == SENT_I).all()
    assert np.array_equal(dst.cpu().numpy(), c["state"])  # (read only)
    return [o[:n] for o in out]


def _reference_call(c, calls=1):
    d, s = c["desired"].copy(), c["start"].copy()
    legs, sw = np.zeros(len(d), np.int32), np.full(len(d), SENT_I, np.int32)
    for _ in range(calls):
        PR.transition(c["state"], d, s, c["threshold"], c["dim"], c["z_2d"], legs, sw)
    return d, s, legs, sw


def test_the_constructed_table_on_the_device(api, torch_cuda, solver):
    for c in Cs.table():
        got, want = _device_call(torch_cuda, solver, c, c["calls"]), _reference_call(c, c["calls"])
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes(), c["name"]
        assert got[3].tolist() == c["expect"].tolist(), c["name"]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
def test_patrol_device_equals_the_restatement(api, torch_cuda, solver, n):
    for dim in (2, 3):
        c = Cs.batch(n, seed=100 + n, dim=dim)
        got, want = _device_call(torch_cuda, solver, c, 2), _reference_call(c, 2)  # (two calls: legs accumulate, swapped is rewritten)
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes(), (n, dim)
        if n >= 63:  # both ways in the first call, and some turn again in the second
            assert 0 < PR.turns(c["state"], c["desired"], c["threshold"], dim, c["z_2d"]).sum() < n and 0 < want[3].sum() and (want[2] == 2).any()


def test_swapped_is_rewritten_when_nobody_turns(api, torch_cuda, solver):
    """A stale 1 in the flag word would exchange the fields again on the next replay."""
    c = Cs.batch(65, seed=5)
    c["threshold"] = 0.0
    n = len(c["state"])
    dd, ds, dl = _dev(torch_cuda, c["desired"]), _dev(torch_cuda, c["start"]), _dev(torch_cuda, np.zeros(n, np.int32))
    dw = _dev(torch_cuda, np.ones(n, np.int32))
    solver.patrol_device(n, _dev(torch_cuda, c["state"]), dd, ds, 0.0, 2, c["z_2d"], dl, dw)
    torch_cuda.cuda.synchronize()
    assert not dw.cpu().numpy().any() and not dl.cpu().numpy().any()
    assert dd.cpu().numpy().tobytes() == c["desired"].tobytes() and ds.cpu().numpy().tobytes() == c["start"].tobytes()


def _code(a, node, which):
    return (which << 30) | (a << 20) | node  # (agent < 1024, node < 2^20)


def _flags(kind, n):
    f = np.zeros(n, np.int32)
    if kind == "all":
        f[:] = 1
    elif kind == "first":
        f[0] = 1
    elif kind == "last":
        f[-1] = 1
    elif kind == "alternating":
        f[::2] = 1
    return f


@pytest.mark.parametrize("nodes", [1, 35, CHUNK - 1, CHUNK, CHUNK + 1])
@pytest.mark.parametrize("n", [1, 2, 257])
def test_field_exchange_on_synthetic_fields(api, torch_cuda, solver, n, nodes):
    """Words that encode (agent, node, which buffer); guard words in front of and behind all four buffers (an odd guard in front, so that the
    slices are 4-byte aligned only)."""
    torch = torch_cuda
    G = 3
    a_idx, node_idx = np.meshgrid(np.arange(n), np.arange(nodes), indexing="ij")
    F = [(_code(a_idx, node_idx, w)).astype(np.int32).reshape(-1) for w in (0, 1)]
    D = [(np.arange(n) * 2 + w + 1000).astype(np.int32) for w in (0, 1)]

    def guarded(a):
        return np.concatenate([np.full(G, SENT_I, np.int32), a, np.full(G, SENT_I, np.int32)])

    for kind in ("none", "all", "first", "last", "alternating"):
        flags = _flags(kind, n)
        bufs = [_dev(torch, guarded(x)) for x in (F[0], F[1], D[0], D[1])]
        dflags = _dev(torch, guarded(flags))
        solver.field_exchange_device(n, nodes, dflags[G:], bufs[0][G:], bufs[1][G:], bufs[2][G:], bufs[3][G:])
        torch.cuda.synchronize()
        out = [b.cpu().numpy() for b in bufs]
        for o in out:
            assert (o[:G] == SENT_I).all() and (o[-G:] == SENT_I).all(), (kind, "guard")
        assert np.array_equal(dflags.cpu().numpy(), guarded(flags))
        f0, f1, d0, d1 = (o[G:-G] for o in out)
        m = flags.astype(bool)
        mw = np.repeat(m, nodes)
        assert np.array_equal(f0, np.where(mw, F[1], F[0])) and np.array_equal(f1, np.where(mw, F[0], F[1])), kind
        assert np.array_equal(d0, np.where(m, D[1], D[0])) and np.array_equal(d1, np.where(m, D[0], D[1])), kind
