// lscpost_traj.hpp — Trajectory::getStateAt's position on the device (reference src/trajectory.cpp:111-170), shared by the kernels that
// sample a plan: the safety figures (lscpost.hip) and the mission record (lscrecord.hip) evaluate the same points with the same code.
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

}  // namespace lscpost
