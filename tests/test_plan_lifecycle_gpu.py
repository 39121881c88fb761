"""The life of a plan's options (lscqp_plan_set_missions / _set_worlds / _set_obstacles / _set_record): a plan on which each was set, replaced
and cleared flies what a plan that only ever saw the final configuration flies, bit for bit; and a step of a plan that waits for
lscqp_plan_reset is refused with the text of the first setter in the order missions, record, obstacles, worlds -- before anything is captured.
The smallest shape that has every option: the 2-D forest worlds, 4 agents in 2 missions of 2, M = 5, 3 row slots, 1 obstacle,
safety_samples = 2, grid waypoints, closed loop."""
import numpy as np
import pytest

from tests import waypoint_device as WD
from tests import world_cases as WLD

pytestmark = pytest.mark.gpu
SIZES = [2, 2]
OFF2 = [0, 1, 4]  # another partition of the same count: agents 1 .. 3 are mission 1


def _setup(api):
    g = WLD.fixture()
    W = WLD.world(0, g)
    sol = api.Solver(api.make_desc(M=5, dim=2, dt=0.2, world_min=W["world_min"], world_max=W["world_max"]))
    maps = [api.WorldMap(g["worlds"][k], W["world_min"], W["world_max"], W["resolution"], W["max_dist"]) for k in range(2)]
    off, starts, goals = WLD.seeded_missions(SIZES, seed=2, g=g, free_everywhere=True)  # (free in both worlds: any partition may fly them)
    z = W["z_2d"]
    one = api.obstacle_models([dict(type="straight", start=[-4.0, 3.0, z], goal=[4.0, -3.0, z], size=0.2, speed=0.6, max_acc=1.0)])
    two = api.obstacle_models([dict(type="straight", start=[-4.0, 3.0, z], goal=[4.0, -3.0, z], size=0.2, speed=0.6, max_acc=1.0),
                               dict(type="straight", start=[4.0, 4.0, z], goal=[-4.0, -4.0, z], size=0.2, speed=0.4, max_acc=1.0)])
    return dict(W=W, sol=sol, maps=maps, ws=api.Worlds(maps), off=off, starts=starts, goals=goals, one=one, two=two)


def _close(c):
    c["ws"].close()
    for m in c["maps"]:
        m.close()
    c["sol"].close()


def _plan(api, c):
    W, N = c["W"], int(c["off"][-1])
    return api.Plan(c["sol"], c["maps"][0], N, 3, WD.agents(api, W["radius"], N), constraint_mode=api.GEN_CLSC, sfc_mode=api.SFC_FROM_HULL,
                    optimize_goal=True, closed_loop=True, z_2d=W["z_2d"], safety_samples=2, record_time_step=0.1, waypoint_mode=api.WAYPOINT_GRID_PIBT)


def _final(plan, c):
    plan.set_missions(c["off"])
    plan.set_worlds(c["ws"])
    plan.set_obstacles(c["one"])
    plan.set_record(0.1)


def _churned(api, c):
    """Every option set, replaced once, cleared with its null form, and set to the final configuration."""
    plan = _plan(api, c)
    _final(plan, c)
    plan.set_missions(OFF2)
    plan.set_worlds(c["ws"])  # (the same worlds again)
    plan.set_obstacles(c["two"])
    plan.set_record(0.25)
    plan.set_record(None)
    plan.set_obstacles(None)
    plan.set_worlds(None)
    plan.set_missions(None)  # (last: a plan with two worlds keeps two missions)
    _final(plan, c)
    return plan


def _state(api, plan):
    """Every public plan buffer, the obstacle table, clock and safety figures, and the mission records, as bytes."""
    out = {b: np.ascontiguousarray(plan.get(b)).tobytes() for b in range(19)}
    for which in (api.PLAN_OBS_TABLE, api.PLAN_OBS_SAFETY, api.PLAN_OBS_CLOCK):
        out["obstacles", which] = plan.get_obstacles(which).tobytes()
    rec, dist = plan.record().download()
    out["record"], out["distance"] = rec.tobytes(), dist.tobytes()
    return out


def _fly(api, torch, plan, c):
    """Reset, then 6 replans: 3 eager, 3 through the graph.  (states after every replan, graph nodes)"""
    plan.reset(c["starts"], c["goals"])
    trace = []
    for t in range(6):
        plan.step(graph=t >= 3)
        torch.cuda.synchronize()
        trace.append(_state(api, plan))
    return trace, plan.graph_nodes()


def _differing(a, b):
    return [(t, k) for t, (x, y) in enumerate(zip(a, b)) for k in x if x[k] != y[k]]


def test_a_churned_plan_flies_what_a_fresh_plan_flies(api, torch_cuda):
    c = _setup(api)
    churned = _churned(api, c)
    fresh = _plan(api, c)
    _final(fresh, c)
    got, nodes = _fly(api, torch_cuda, churned, c)
    want, want_nodes = _fly(api, torch_cuda, fresh, c)
    assert not _differing(got, want)
    assert nodes == want_nodes and nodes > 0
    assert churned.missions().tolist() == list(c["off"]) and churned.n_dyn == 1 and len(fresh.get_obstacles()) == 1
    moved = np.frombuffer(want[-1][api.PLAN_STATE], np.float64).reshape(-1, 9)[:, :2] - np.asarray(c["starts"])[:, :2]
    assert np.abs(moved).max() > 0.05  # (the flight is one: the agents left their start points)
    churned.close()
    fresh.close()
    again = _churned(api, c)  # every owner was released and is built again
    got, nodes = _fly(api, torch_cuda, again, c)
    assert not _differing(got, want) and nodes == want_nodes
    again.close()
    _close(c)


def test_step_refusals_keep_their_order(api, torch_cuda):
    torch = torch_cuda
    c = _setup(api)

    def refused(graph, text):
        with pytest.raises(api.LscqpError) as e:
            plan.step(graph=graph)
        assert e.value.code == api.ERR_INVALID_ARGUMENT and str(e.value).count("lscqp_plan_reset must come") == 1 and text in str(e.value), str(e.value)
        # nothing was captured and nothing is being captured: a synchronous copy is legal and the graph is the one there was
        assert not torch.cuda.is_current_stream_capturing()
        plan.get(api.PLAN_STATE)

    plan = _plan(api, c)
    plan.set_missions(c["off"])
    plan.reset(c["starts"], c["goals"])
    plan.step()
    plan.step(graph=True)  # (past the first replan: a graph step is a graph step from here on)
    torch.cuda.synchronize()
    assert plan.graph_nodes() > 0
    plan.set_obstacles(c["one"])
    plan.set_missions(OFF2)  # missions and obstacles both pending: the missions speak first
    assert plan.graph_nodes() == 0
    for graph in (False, True):
        refused(graph, "lscqp_plan_set_missions: lscqp_plan_reset must come before the next step")
    assert plan.graph_nodes() == 0
    plan.reset(c["starts"], c["goals"])
    plan.step()
    plan.step(graph=True)
    torch.cuda.synchronize()
    plan.set_worlds(c["ws"])
    for graph in (False, True):
        refused(graph, "lscqp_plan_set_worlds: lscqp_plan_reset must come before the next step")
    plan.reset(c["starts"], c["goals"])
    plan.step()  # (the next eager step after a reset succeeds, and the graph after it)
    plan.step(graph=True)
    torch.cuda.synchronize()
    assert plan.graph_nodes() > 0
    plan.close()
    _close(c)
