"""lscqp_plan_set_waypoint_decision: a plan whose chain starts with the wide form of the waypoint decision flies bit for bit what a plan
left at the default flies, eagerly and through the captured graph; where the setter is refused the plan stays as it was."""
import numpy as np
import pytest

from tests import waypoint_cases as WC
from tests import waypoint_device as WD

pytestmark = pytest.mark.gpu


def _snapshot(api, plan):
    """Every buffer of the plan, the records as raw bytes."""
    raw = (api.PLAN_HEADER, api.PLAN_ROWS, api.PLAN_SFC, api.PLAN_INFO, api.PLAN_SAFETY)
    return [plan.get(b).view(np.uint8).copy() if b in raw else plan.get(b).copy() for b in range(19)]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_forest10_flies_the_same_with_the_wide_decision(api, torch_cuda):
    """79 replans of forest10: default decision and WIDE, eager and graph -- four flights, every buffer equal replan by replan."""
    import torch

    W = WC.forest10()
    starts, goals = np.array(W["starts"], float), np.array(W["goals"], float)
    flights, nodes = {}, {}
    for decision in (api.DECISION_ONE_WORKGROUP, api.DECISION_WIDE):
        for graph in (False, True):
            sol, wmap, plan = WD.forest10_plan(api, W)
            if decision != api.DECISION_ONE_WORKGROUP:
                plan.set_waypoint_decision(decision)
            plan.reset(starts, goals)
            trace = []
            for _ in range(79):
                plan.step(graph=graph)
                torch.cuda.synchronize()
                trace.append(_snapshot(api, plan))
            assert plan.grid().status() == 0
            flights[decision, graph], nodes[decision, graph] = trace, plan.graph_nodes()
            plan.close()
            wmap.close()
    base = flights[api.DECISION_ONE_WORKGROUP, False]
    assert sum(int(t[api.PLAN_WAYPOINT_UPDATED].sum()) for t in base) > 100  # (the decision does move waypoints along this flight)
    for key, trace in flights.items():
        for k in range(79):
            assert _same(base[k], trace[k]), (key, k)
    assert nodes[api.DECISION_ONE_WORKGROUP, False] == 0 and nodes[api.DECISION_WIDE, False] == 0
    # (range 3 m: the wide form is eleven launches where the one-workgroup form is two)
    assert nodes[api.DECISION_WIDE, True] == nodes[api.DECISION_ONE_WORKGROUP, True] + 9, nodes


def test_graph_node_count_survives_resets(api, torch_cuda):
    import torch

    W = WC.forest10()
    starts, goals = np.array(W["starts"], float), np.array(W["goals"], float)
    sol, wmap, plan = WD.forest10_plan(api, W)
    plan.set_waypoint_decision(api.DECISION_WIDE)
    counts = []
    for g in (goals, goals[::-1].copy(), np.roll(goals, 3, axis=0)):
        plan.reset(starts, g)
        for _ in range(2):
            plan.step(graph=True)
        torch.cuda.synchronize()
        assert (plan.get(api.PLAN_STATUS) == 0).all()
        counts.append(plan.graph_nodes())
    assert counts[0] > 0 and counts[0] == counts[1] == counts[2], counts
    plan.close()
    wmap.close()


def test_auto_picks_the_form_by_agent_count(api, torch_cuda):
    """AUTO on ten agents (below the threshold) is the one-workgroup chain node for node."""
    import torch

    W = WC.forest10()
    assert len(W["starts"]) < api.DECISION_AUTO_MIN_AGENTS
    starts, goals = np.array(W["starts"], float), np.array(W["goals"], float)
    nodes = {}
    for decision in (api.DECISION_ONE_WORKGROUP, api.DECISION_AUTO):
        sol, wmap, plan = WD.forest10_plan(api, W)
        plan.set_waypoint_decision(decision)
        plan.reset(starts, goals)
        for _ in range(2):
            plan.step(graph=True)
        torch.cuda.synchronize()
        nodes[decision] = plan.graph_nodes()
        plan.close()
        wmap.close()
    assert nodes[api.DECISION_AUTO] == nodes[api.DECISION_ONE_WORKGROUP] > 0


def test_setter_is_refused_without_the_grid_planner(api, torch_cuda):
    W = WC.forest10()
    sol, wmap, plan = WD.forest10_plan(api, W, waypoint_mode=api.WAYPOINT_FROM_CALLER)
    for decision in (api.DECISION_ONE_WORKGROUP, api.DECISION_WIDE, api.DECISION_AUTO):
        with pytest.raises(api.LscqpError) as e:
            plan.set_waypoint_decision(decision)
        assert e.value.code == api.ERR_INVALID_ARGUMENT and "LSCQP_WAYPOINT_FROM_CALLER" in str(e.value)
    plan.close()
    sol, wmap2, plan = WD.forest10_plan(api, W)
    with pytest.raises(api.LscqpError) as e:
        plan.set_waypoint_decision(7)
    assert e.value.code == api.ERR_INVALID_ARGUMENT
    plan.close()
    wmap2.close()
    wmap.close()


@pytest.mark.parametrize("first", ["partition", "decision"])
def test_setter_and_a_partition_refuse_each_other(api, torch_cuda, first):
    """A partition of K > 1 missions keeps one workgroup per mission: whichever of the two is set first, the other is refused with
    LSCQP_ERR_UNSUPPORTED and the plan is as it was -- one more step still matches a plan that never saw the refused call."""
    import torch

    W = WC.forest10()
    starts, goals = np.array(W["starts"], float), np.array(W["goals"], float)
    kw = dict(mission_offsets=[0, 5, 10]) if first == "partition" else {}
    plans = [WD.forest10_plan(api, W, **kw) for _ in range(2)]
    a, b = plans[0][2], plans[1][2]
    if first == "decision":
        b.set_waypoint_decision(api.DECISION_WIDE)
    for p in (a, b):
        p.reset(starts, goals)
        for _ in range(3):
            p.step(graph=True)
    torch.cuda.synchronize()
    assert _same(_snapshot(api, a), _snapshot(api, b))
    nodes = b.graph_nodes()
    if first == "partition":
        for decision in (api.DECISION_WIDE, api.DECISION_AUTO):
            with pytest.raises(api.LscqpError) as e:
                b.set_waypoint_decision(decision)
            assert e.value.code == api.ERR_UNSUPPORTED
        assert b.missions().tolist() == [0, 5, 10]
    else:
        with pytest.raises(api.LscqpError) as e:
            b.set_missions([0, 5, 10])
        assert e.value.code == api.ERR_UNSUPPORTED
        assert b.missions().tolist() == [0, 10]
    assert b.graph_nodes() == nodes  # (the captured graph was not dropped either)
    for p in (a, b):
        p.step(graph=True)
    torch.cuda.synchronize()
    assert _same(_snapshot(api, a), _snapshot(api, b))
    if first == "partition":
        b.set_waypoint_decision(api.DECISION_ONE_WORKGROUP)  # (the default is always accepted)
    for _, wmap, p in plans:
        p.close()
        wmap.close()


def test_setter_works_with_a_single_mission_partition(api, torch_cuda):
    import torch

    W = WC.forest10()
    starts, goals = np.array(W["starts"], float), np.array(W["goals"], float)
    plans = [WD.forest10_plan(api, W) for _ in range(2)]
    a, b = plans[0][2], plans[1][2]
    b.set_missions([0, 10])
    b.set_waypoint_decision(api.DECISION_WIDE)
    b.set_missions([0, 10])  # (and the other way round)
    for p in (a, b):
        p.reset(starts, goals)
        for _ in range(5):
            p.step(graph=True)
    torch.cuda.synchronize()
    assert _same(_snapshot(api, a), _snapshot(api, b))
    assert b.graph_nodes() == a.graph_nodes() + 9
    for _, wmap, p in plans:
        p.close()
        wmap.close()
