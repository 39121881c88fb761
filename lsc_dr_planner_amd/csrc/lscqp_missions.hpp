// lscqp_missions.hpp — a mission partition as the kernels read it (include/lscqp.h, "many missions over one map"): off[0..K], strictly
// increasing from 0 to the number of agents, on the device.
#pragma once
#include <stdint.h>

namespace lscqp_missions {

// the mission of agent a: the k with off[k] <= a < off[k + 1]
__device__ __forceinline__ int mission_of(const int64_t* __restrict__ off, int K, int64_t a) {
    int k0 = 0, k1 = K - 1;
    while (k0 < k1) {
        const int mid = (k0 + k1 + 1) >> 1;
        if (off[mid] <= a) k0 = mid;
        else k1 = mid - 1;
    }
    return k0;
}

}  // namespace lscqp_missions
