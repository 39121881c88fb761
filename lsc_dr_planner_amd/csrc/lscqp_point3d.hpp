// lscqp_point3d.hpp — the one piece of octomath::Vector3 arithmetic that two units evaluate alike: the mission record's finish test
// (lscrecord.hip) and the patrol transition (lscpatrol.hip) measure an agent's distance to its desired goal with the same function, so a
// GOTO mission and a patrol agree on every bit of it and differ only in how they compare it with goal_threshold.
#ifndef LSCQP_POINT3D_HPP
#define LSCQP_POINT3D_HPP

#include <hip/hip_runtime.h>
#include <math.h>

namespace lscqp {

// (a - b).norm() of octomath::Vector3: float differences, float sum of squares, the square root of that value in double
__host__ __device__ __forceinline__ double norm_of_difference(const float (&a)[3], const float (&b)[3]) {
#pragma clang fp contract(off)
    const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    const float nsq = dx * dx + dy * dy + dz * dz;
    return sqrt((double)nsq);
}

}  // namespace lscqp

#endif  // LSCQP_POINT3D_HPP
