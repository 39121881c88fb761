"""What the GPU tests of the waypoint layer share (test_waypoints_gpu, test_waypoints_wide_gpu, test_waypoints_wide_plan_gpu,
test_missions_gpu): a world on the device, its fields, one decision by any of the three entries, and the forest10 plan.  Plain functions that
take `torch` / `api` as arguments; the cases themselves are in waypoint_cases.py and mission_cases.py."""
import os
import sys

import numpy as np

from tests import waypoint_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def closed_loop():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import closed_loop

    return closed_loop


def dev(torch, a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda")


def device_grid(api, w, resolution=0.5):
    wmap = api.WorldMap(w["boxes"], w["world_min"], w["world_max"], w["resolution"], w["max_dist"])
    return wmap, api.Grid(wmap, resolution, w["radius"], w["z_2d"])


def device_fields(torch, grid, starts, goals):
    f, d = grid.fields(dev(torch, starts, np.float64), dev(torch, goals, np.float64))
    torch.cuda.synchronize()
    return f, d


def decision_step(torch, grid, rng, s, d_field, d_init_d, M=10, wide=False, off=None):
    """(group, desired, updated, new waypoints) of one decision over the state s (positions, plans, current_goals, waypoints; positions ride
    in a state record): lscqp_waypoints_device, lscqp_waypoints_wide_device (wide) or lscqp_waypoints_missions_device (off: the partition).
    No walk may have reached its bound."""
    n = len(s["waypoints"])
    st = np.zeros((n, 9))
    st[:, :3] = s["positions"]
    d_way = dev(torch, s["waypoints"], np.float64)
    d_plan = None if s["plans"] is None else dev(torch, WC.plan_from_points(np.asarray(s["plans"])), np.float64)
    args = (rng, M, 2, dev(torch, st), d_plan, dev(torch, s["current_goals"], np.float64), d_field, d_init_d, d_way)
    if off is not None:
        g, d, u = grid.waypoints_missions(off, *args)
    else:
        g, d, u = (grid.waypoints_wide if wide else grid.waypoints)(*args)
    torch.cuda.synchronize()
    if off is not None:
        assert not grid.mission_status(len(off) - 1).any()
    else:
        assert grid.status() == 0
    return g.cpu().numpy(), d.cpu().numpy(), u.cpu().numpy(), d_way.cpu().numpy().reshape(n, 3)


def agents(api, radius, N):
    ag = np.zeros(N, api.AGENT_PARAM_DTYPE)
    ag["radius"], ag["downwash"], ag["max_vel"], ag["max_acc"], ag["nominal_velocity"] = radius, 2.0, 1.0, 2.0, 1.0
    return ag


def forest10_plan(api, W, waypoint_mode=1, **kw):
    N = len(W["starts"])
    sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, world_min=W["world_min"], world_max=W["world_max"]))
    wmap = api.WorldMap(W["boxes"], W["world_min"], W["world_max"], W["resolution"], W["max_dist"])
    plan = api.Plan(sol, wmap, N, N - 1, agents(api, W["radius"], N), constraint_mode=api.GEN_CLSC, sfc_mode=api.SFC_FROM_HULL, optimize_goal=True, closed_loop=True,
                    z_2d=W["z_2d"], safety_samples=2, record_time_step=0.1, waypoint_mode=waypoint_mode, **kw)
    return sol, wmap, plan
