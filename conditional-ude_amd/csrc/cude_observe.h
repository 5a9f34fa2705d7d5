// What the kernels around the replicate simulations state once (cude_predictive.hip, cude_bootstrap.hip, cude_npde.hip,
// cude_vpc.hip): a simulated observation, and the test that a value is neither NaN nor infinite.
#pragma once
#include <hip/hip_runtime.h>

namespace cude {

__device__ __forceinline__ bool finite_value(double v) { return fabs(v) <= 1.79769313486231570815e308; }

// v + (sigma s) eps, every operation rounded on its own (no contraction), so that numpy's expression has the same bits and a
// caller can rebuild a replicate's data from public outputs (cude_bootstrap_conditional rule 2, cude_npde rule 4)
__device__ __forceinline__ double simulated_observation(double v, double sigma, double scale, double eps) {
#pragma clang fp contract(off)
    const double amp = sigma * scale;
    const double d = amp * eps;
    return v + d;
}

}  // namespace cude
