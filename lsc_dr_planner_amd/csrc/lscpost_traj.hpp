// lscpost_traj.hpp — Trajectory::getStateAt's position on the device (reference src/trajectory.cpp:111-170), shared by the kernels that
// sample a plan: the safety figures (lscpost.hip) and the mission record (lscrecord.hip) evaluate the same points with the same code.
// state_at is the whole sampled state -- position, velocity, acceleration -- for the record's flight log.
#pragma once
#include <hip/hip_runtime.h>

namespace lscpost {

// sum_i cp[i] C(n,i) t^i (1-t)^(n-i)
template <int N>
__device__ __forceinline__ double bern(const double (&cp)[6], double t) {
    constexpr int binom[6][6] = {{1, 0, 0, 0, 0, 0}, {1, 1, 0, 0, 0, 0}, {1, 2, 1, 0, 0, 0}, {1, 3, 3, 1, 0, 0}, {1, 4, 6, 4, 1, 0}, {1, 5, 10, 10, 5, 1}};
    double s = 0, ti = 1;
    double omt[6];
    omt[0] = 1;
#pragma unroll
    for (int i = 1; i <= N; i++) omt[i] = omt[i - 1] * (1 - t);
#pragma unroll
    for (int i = 0; i <= N; i++) {
        s += cp[i] * binom[N][i] * ti * omt[N - i];
        ti *= t;
    }
    return s;
}

// position (float32, as State holds it) of the trajectory xq at time t
__device__ __forceinline__ void position_at(int M, int dim, double dt, double t, double z_2d, const double* xq, float (&pos)[3]) {
    const int P = 6 * M;
    int ms = -1;
    double tn = 0, end = 0;
    for (int idx = 0; idx < M; idx++) {  // getPointAt's segment search (src/trajectory.cpp:121-136)
        end += dt;
        if (t < end) {
            ms = idx;
            tn = 1 - (end - t) / dt;
            break;
        }
    }
    if (ms < 0) {
        ms = M - 1;
        tn = 1.0;
    }
    for (int k = 0; k < 3; k++) {
        double c[6];
        for (int i = 0; i < 6; i++) c[i] = (k < dim) ? (double)(float)xq[k * P + 6 * ms + i] : (double)(float)z_2d;
        pos[k] = (float)bern<5>(c, tn);
    }
}

// Trajectory::getStateAt whole: position, velocity and acceleration (float32 each, as State holds them) of the trajectory xq at time t.
// The segment search and the position are position_at's; the derivative control points are formed as the safety figures form them
// (lscpost.hip: derivative(), src/trajectory.cpp:183-199).  Axes k >= dim: z_2d, at rest (doStep, src/agent_manager.cpp:40-42).
__device__ __forceinline__ void state_at(int M, int dim, double dt, double t, double z_2d, const double* xq, float (&pos)[3], float (&vel)[3],
                                         float (&acc)[3]) {
    const int P = 6 * M;
    int ms = -1;
    double tn = 0, end = 0;
    for (int idx = 0; idx < M; idx++) {
        end += dt;
        if (t < end) {
            ms = idx;
            tn = 1 - (end - t) / dt;
            break;
        }
    }
    if (ms < 0) {
        ms = M - 1;
        tn = 1.0;
    }
    for (int k = 0; k < 3; k++) {
        if (k >= dim) {
            pos[k] = (float)z_2d, vel[k] = 0.0f, acc[k] = 0.0f;
            continue;
        }
        double c[6], d1[6] = {0, 0, 0, 0, 0, 0}, d2[6] = {0, 0, 0, 0, 0, 0};
        for (int i = 0; i < 6; i++) c[i] = (double)(float)xq[k * P + 6 * ms + i];
        for (int i = 0; i < 5; i++) d1[i] = (c[i + 1] - c[i]) * (5.0 / dt);
        for (int i = 0; i < 4; i++) d2[i] = (d1[i + 1] - d1[i]) * (4.0 / dt);
        pos[k] = (float)bern<5>(c, tn);
        vel[k] = (float)bern<4>(d1, tn);
        acc[k] = (float)bern<3>(d2, tn);
    }
}

}  // namespace lscpost
