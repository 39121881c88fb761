// flight_log_csv.cpp — SimulationResultCsv::writeFlight from a host (tests/test_flight_log_cpu.py): argv[1] holds, in text, "qn on n_replans
// n_samples t0 time_step record_time_step", then the states [n_replans][qn][n_samples][9], the obstacle rows [n_replans][on][4] and the
// planning times [n_replans][qn] of one mission's downloaded flight log; the header and the rows go to stdout.
#include <fstream>
#include <iostream>
#include <vector>

#include "result_csv.hpp"

using namespace DynamicPlanning;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    size_t qn = 0, on = 0, n_replans = 0, n_samples = 0;
    double t0 = 0, time_step = 0, record_time_step = 0;
    if (!(in >> qn >> on >> n_replans >> n_samples >> t0 >> time_step >> record_time_step)) return 3;
    std::vector<float> states(n_replans * qn * n_samples * 9), obstacles(n_replans * on * 4);
    std::vector<double> planning_time(n_replans * qn);
    for (float& v : states)
        if (!(in >> v)) return 4;
    for (float& v : obstacles)
        if (!(in >> v)) return 5;
    for (double& v : planning_time)
        if (!(in >> v)) return 6;
    SimulationResultCsv csv(std::cout, qn, on);
    csv.writeHeader();
    csv.writeFlight(t0, time_step, record_time_step, n_replans, n_samples, states.data(), on ? obstacles.data() : nullptr, planning_time);
    return 0;
}
