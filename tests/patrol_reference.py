"""Plain numpy restatement of the PATROL branch of the reference's planning state transition, written from its source: the test-side
reference of lscqp_patrol_device / lscqp_patrol_host (include/lscqp.h, "patrol missions").

    AgentManager::planningStateTransition     src/agent_manager.cpp:225-240
    octomath::Vector3::distance               float32 differences, a float32 sum of squares, the square root in double

    } else if (planner_state == PlannerState::PATROL and
               agent.desired_goal_point.distance(agent.current_state.position) < param.goal_threshold) {
        point3d temp = agent.desired_goal_point;
        agent.desired_goal_point = agent.start_point;
        agent.start_point = temp;
    }

This file DEFINES the arithmetic: every float32 operation is rounded on its own (numpy scalars never contract a multiply and an add), the
comparison is in double and strict.  Nothing here shares code with the product."""
import math

import numpy as np

f32 = np.float32


def distance(goal, position):
    """goal.distance(position) of two points held in double: each narrowed to float32 first."""
    s = f32(0)
    sq = []
    for k in range(3):
        e = f32(f32(goal[k]) - f32(position[k]))
        sq.append(f32(e * e))
    s = f32(f32(sq[0] + sq[1]) + sq[2])
    return math.sqrt(float(s))


def position_of(state_row, dim, z_2d):
    """agent.current_state.position as the transition sees it: the state buffer's words, and the mission's plane for a 2-D class."""
    return [state_row[0], state_row[1], state_row[2] if dim == 3 else z_2d]


def transition(state, desired, start, goal_threshold, dim, z_2d, legs, swapped):
    """One call over every agent, in place like the entries: state (n, 9), desired / start (n, 3) float64, legs / swapped (n,) int32."""
    for a in range(len(state)):
        turn = distance(desired[a], position_of(state[a], dim, z_2d)) < float(goal_threshold)
        if turn:
            t = desired[a].copy()
            desired[a] = start[a]
            start[a] = t
            legs[a] += 1
        swapped[a] = 1 if turn else 0


def turns(state, desired, goal_threshold, dim, z_2d):
    """Who would turn, without changing anything: bool (n,)."""
    return np.array([distance(desired[a], position_of(state[a], dim, z_2d)) < float(goal_threshold) for a in range(len(state))], bool)
