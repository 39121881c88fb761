// record_obstacle_summary.cpp — the two forms of fillSummaryFromRecord from a host (tests/test_record_obstacles_cpu.py): the 28 fields of a
// summary line come from the file argv[1] (one per line), a mission record's flight figures from argv[2..4] -- flight_time, distance,
// safety_ratio_agent -- and an obstacle record's safety_ratio_obs from argv[5].  Two rows go to stdout: the line filled by the
// two-argument form (safety_ratio_obs stays the file's), then by the three-argument form (safety_ratio_obs is the obstacle record's).
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "result_csv.hpp"

using namespace DynamicPlanning;

int main(int argc, char** argv) {
    if (argc != 6) return 2;
    std::ifstream in(argv[1]);
    std::vector<std::string> f;
    for (std::string line; std::getline(in, line);) f.push_back(line);
    if (f.size() != 28) return 3;
    auto d = [&](int i) { return std::atof(f[i].c_str()); };
    SimulationSummary s;
    s.start_time = f[0];
    s.safety_ratio_obs = d(4);
    double* times[] = {&s.mapf_time_average, &s.mapf_time_min, &s.mapf_time_max, &s.planning_time_average, &s.planning_time_min, &s.planning_time_max,
                       &s.initial_traj_planning_time, &s.obstacle_prediction_time, &s.goal_planning_time, &s.lsc_generation_time, &s.sfc_generation_time,
                       &s.traj_optimization_time};
    for (int i = 0; i < 12; i++) *times[i] = d(7 + i);
    s.mission_file_name = f[19], s.world_file_name = f[20], s.planner_mode = f[21], s.goal_mode = f[22], s.mapf_mode = f[23];
    s.communication_range = d(24), s.world_dimension = std::atoi(f[25].c_str()), s.M = std::atoi(f[26].c_str()), s.dt = d(27);
    lscqp_mission_record r = {};
    r.flight_time = std::atof(argv[2]), r.distance = std::atof(argv[3]), r.safety_ratio_agent = std::atof(argv[4]);
    lscqp_mission_obstacle_record o = {};
    o.safety_ratio_obs = std::atof(argv[5]);
    o.replan = o.agent = o.obstacle = o.sample = -1;
    static_assert(sizeof(lscqp_mission_obstacle_record) == 40 && sizeof(lscqp_agent_obstacle_record) == 24, "include/lscqp.h: the obstacle record's structs");
    SimulationSummary two = s, three = s;
    fillSummaryFromRecord(two, r);
    fillSummaryFromRecord(three, r, o);
    SimulationSummaryCsv::writeRow(std::cout, two);
    SimulationSummaryCsv::writeRow(std::cout, three);
    return 0;
}
