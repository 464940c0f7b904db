// The glue of a batch of Darcy conditioning problems (scripts/darcy/solve_darcy_gmrf-fem.jl:176-198 per problem) that is not
// already a kernel of the element assembly, the posterior assembly, the factor or the variance estimators: the last line of the
// loop body,
//     std = sqrt(var),     norm(std)                                                                  (:192, :196)
// for B problems at once.  All arrays are problem-major; blockIdx.y is the problem.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "selinv.hpp"

namespace gmrf {

// v[p][i] <- sqrt(v[p][i]) in place and part[p][c] = sum of the new v[p][i]^2 over the rows [c len, (c + 1) len).  The partition
// depends on n only, thread t takes the rows t, t + 256, ... of its chunk in order and the workgroup adds its 256 sums in a fixed
// tree (gn_objective_part / pattern_dot_part do the same): no atomics, and a problem's value does not depend on the batch it
// sits in.  std_norm_finish adds a problem's chunks with pattern_dot_sum's tree and takes the root.
__global__ __launch_bounds__(256) void std_norm_part(double* __restrict__ v, int64_t n, int64_t len, double* __restrict__ part) {
    __shared__ double red[256];
    const int64_t c = blockIdx.x, p = blockIdx.y, nch = gridDim.x;
    v += p * n;
    double acc = 0.0;
    const int64_t i1 = min(n, (c + 1) * len);
    for (int64_t i = c * len + threadIdx.x; i < i1; i += 256) {
        const double s = sqrt(v[i]);
        v[i] = s;
        acc = fma(s, s, acc);
    }
    const double sum = block_sum_256(acc, red);
    if (threadIdx.x == 0) part[p * nch + c] = sum;
}

__global__ __launch_bounds__(256) void std_norm_finish(const double* __restrict__ part, int64_t nch, double* __restrict__ out) {
    __shared__ double red[256];
    const int64_t p = blockIdx.y;
    const double* q = part + p * nch;
    double acc = 0.0;
    for (int64_t c = threadIdx.x; c < nch; c += 256) acc += q[c];
    const double sum = block_sum_256(acc, red);
    if (threadIdx.x == 0) out[p] = sqrt(sum);
}

}  // namespace gmrf
