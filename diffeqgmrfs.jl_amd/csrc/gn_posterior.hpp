// The scores of the posterior stage of a batch of Gauss-Newton loops (scripts/burgers/solve_burgers_gmrf-collocation.jl:208-215,
// :262-263 per problem) that are not already a kernel of the factor, the samplers or the variance estimators:
//     logdet(A_p),     sqmahal_p = (z_p - x_p)' A_p (z_p - x_p),     nll_p = 0.5 (n log(2 pi) + sqmahal_p - logdet(A_p))
// for B problems at once.  All arrays are problem-major; blockIdx.y is the problem.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "selinv.hpp"

namespace gmrf {

// out[p] = 2 * (part[p][0] + part[p][1] + ... + part[p][N - 1]), one thread per problem, the blocks in order: the sum and the
// product of the host loop of gmrf_bt_logdet, so the same bits.
__global__ __launch_bounds__(256) void logdet_sum_batch(const double* __restrict__ part, int64_t N, int64_t B, double* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= B) return;
    const double* q = part + p * N;
    double s = 0.0;
    for (int64_t i = 0; i < N; ++i) s += q[i];
    out[p] = 2.0 * s;
}

// part[p][c] = sum over the columns j in [c len, (c + 1) len) of d_j (A_p d)_j with d = z_p - x_p, formed as it is read: no d vector
// is written.  A_p is symmetric with both triangles stored, so column j of the CSC arrays (ptr, row) is row j.  One pass over the
// values: 8 + 4 bytes per stored entry plus the two gathered operands.  The partition depends on n only, thread t takes the columns
// t, t + 256, ... of its chunk in order and the workgroup adds its 256 sums in a fixed tree (gn_objective_part / std_norm_part do
// the same): no atomics, and a problem's value does not depend on the batch it sits in.  pattern_dot_sum adds a problem's chunks.
__global__ __launch_bounds__(256) void quadform_part(const int64_t* __restrict__ ptr, const int32_t* __restrict__ row,
                                                     const double* __restrict__ a, int64_t a_stride, const double* __restrict__ x,
                                                     const double* __restrict__ z, int64_t n, int64_t len, double* __restrict__ part) {
    __shared__ double red[256];
    const int64_t c = blockIdx.x, p = blockIdx.y, nch = gridDim.x;
    a += p * a_stride; x += p * n; z += p * n;
    double acc = 0.0;
    const int64_t j1 = min(n, (c + 1) * len);
    for (int64_t j = c * len + threadIdx.x; j < j1; j += 256) {
        double s = 0.0;
        for (int64_t e = ptr[j]; e < ptr[j + 1]; ++e) {
            const int32_t r = row[e];
            s = fma(a[e], z[r] - x[r], s);
        }
        acc = fma(z[j] - x[j], s, acc);
    }
    const double v = block_sum_256(acc, red);
    if (threadIdx.x == 0) part[p * nch + c] = v;
}

// nll[p] = 0.5 * ((n * log2pi + sqmahal[p]) - logdet[p]), one thread per problem, every operation rounded on its own (no fused
// multiply-add): the value NumPy gives for the same expression.
__global__ __launch_bounds__(256) void nll_batch(double n, double log2pi, const double* __restrict__ sqmahal,
                                                 const double* __restrict__ logdet, int64_t B, double* __restrict__ out) {
#pragma clang fp contract(off)
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= B) return;
    const double t = n * log2pi;
    out[p] = 0.5 * ((t + sqmahal[p]) - logdet[p]);
}

}  // namespace gmrf
