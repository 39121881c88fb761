"""The prescreen inside lscqp_plan's chain: one node more in the captured graph than the chain with the phase and its interior-point pass as
two launches, the mission's buffers unchanged, and the setter reaching a live plan (the graph is dropped and captured again, as after
lscqp_update)."""
import numpy as np
import pytest

from tests.test_plan import _make_plan, _mission

REPLANS = 20


def _buffers(api, plan):
    return {w: plan.get(w).copy() for w in (api.PLAN_PLAN, api.PLAN_GOAL, api.PLAN_STATUS, api.PLAN_GOAL_STATUS, api.PLAN_VALID, api.PLAN_NEXT_STATE,
                                            api.PLAN_OBJECTIVE, api.PLAN_INFO, api.PLAN_IN_RANGE)}


def _fly(api, torch, plan, W, m, graph, replans=REPLANS, starts=None, states=None):
    plan.reset(np.array(W["starts"], dtype=np.float64) if starts is None else starts)
    out = []
    for k in range(replans):
        plan.put(api.PLAN_STATE, m["state"][k] if states is None else states[k])
        plan.put(api.PLAN_WAYPOINT, m["way"][k])
        plan.step(graph=graph)
        torch.cuda.synchronize()
        out.append(_buffers(api, plan))
    return out


def _same(a, b):
    return all(x[w].tobytes() == y[w].tobytes() for x, y in zip(a, b) for w in x)


@pytest.mark.gpu
def test_plan_with_the_prescreen_flies_the_default_plans_mission(api, torch_cuda):
    torch = torch_cuda
    g, W, m = _mission()
    sol0, map0, ref = _make_plan(api, W, m["N"])
    want_e = _fly(api, torch, ref, W, m, graph=False)
    want_g = _fly(api, torch, ref, W, m, graph=True)
    nodes = ref.graph_nodes()
    assert nodes >= 8 and _same(want_e, want_g)
    assert all((b[api.PLAN_STATUS] == 0).all() for b in want_e)
    # the chain the prescreen is added to: the phase and the first interior-point pass as two launches (the one-launch fused form is not
    # used while the prescreen is on) -- what knob das_fused = 0 gives, one node more than the default where the class has a fused form
    sol2, map2, two = _make_plan(api, W, m["N"])
    sol2.set_knob("das_fused", 0)
    assert _same(_fly(api, torch, two, W, m, graph=True, replans=3), want_e[:3])
    nodes_two = two.graph_nodes()
    assert nodes_two in (nodes, nodes + 1)
    two.close()

    sol, wmap, plan = _make_plan(api, W, m["N"])
    sol.set_prescreen(api.PRESCREEN_ON)
    got_e = _fly(api, torch, plan, W, m, graph=False)
    assert plan.graph_nodes() == 0 and _same(got_e, want_e)
    got_g = _fly(api, torch, plan, W, m, graph=True)
    assert _same(got_g, want_e)
    assert plan.graph_nodes() == nodes_two + 1  # the prescreen's launch, and nothing else
    # the setter in the middle of a mission: the captured chain is dropped and captured again, and the mission goes on unchanged
    sol.set_prescreen(api.PRESCREEN_OFF)
    for k in range(REPLANS, REPLANS + 3):
        for p in (ref, plan):
            p.put(api.PLAN_STATE, m["state"][k])
            p.put(api.PLAN_WAYPOINT, m["way"][k])
            p.step(graph=True)
        torch.cuda.synchronize()
        assert plan.graph_nodes() == nodes
        assert _same([_buffers(api, plan)], [_buffers(api, ref)])
    sol.set_prescreen(api.PRESCREEN_ON)
    plan.put(api.PLAN_STATE, m["state"][REPLANS + 3])
    plan.put(api.PLAN_WAYPOINT, m["way"][REPLANS + 3])
    plan.step(graph=True)
    torch.cuda.synchronize()
    assert plan.graph_nodes() == nodes_two + 1
    for p in (ref, plan):
        p.close()


@pytest.mark.gpu
def test_plan_with_two_agents_inside_each_others_model(api, torch_cuda):
    """Two of the ten agents are placed 5 cm apart, far inside each other's collision model.  What that violates is a row at the agents'
    PRESENT position -- the fixed control points, where the reference's QP holds no LSC row (src/traj_optimizer.cpp:404-406) and the prescreen
    therefore gives no verdict: the chain with the prescreen on must do exactly what the default chain does, failsafe included, and whatever
    the prescreen does mark is INFEASIBLE and keeps initial_traj."""
    torch = torch_cuda
    g, W, m = _mission()
    states = m["state"][:6].copy()
    states[:, 1, 0:3] = states[:, 0, 0:3] + np.array([0.05, 0.0, 0.0])
    starts = np.array(W["starts"], dtype=np.float64)
    starts[1] = starts[0] + np.array([0.05, 0.0, 0.0])
    sol0, map0, ref = _make_plan(api, W, m["N"])
    want = _fly(api, torch, ref, W, m, graph=False, replans=6, starts=starts, states=states)
    sol, wmap, plan = _make_plan(api, W, m["N"])
    sol.set_prescreen(api.PRESCREEN_ON)
    got = _fly(api, torch, plan, W, m, graph=False, replans=6, starts=starts, states=states)
    for a, b in zip(got, want):
        flagged = (a[api.PLAN_INFO]["flags"] & api.INFO_PRESCREENED) != 0
        assert (a[api.PLAN_STATUS][flagged] == api.STATUS_INFEASIBLE).all()
        for w in a:
            if w == api.PLAN_INFO:
                assert a[w][~flagged].tobytes() == b[w][~flagged].tobytes()
            else:
                assert a[w].tobytes() == b[w].tobytes(), w
    for p in (ref, plan):
        p.close()
