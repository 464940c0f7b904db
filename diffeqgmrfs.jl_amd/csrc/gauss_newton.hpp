// The glue of a batch of Gauss-Newton loops (scripts/solve_burger.jl:151-180 per problem) on the device: the objective
//     obj = (x_prior - x)' Q (x_prior - x) + noise |obs_diff|^2                                   (:157, :163-168)
// and the stop rule of :161 / :171.  B problems on one mesh advance in lock step; nothing but one word ("problems still active")
// crosses the bus per iteration.  All arrays are problem-major; blockIdx.y is the problem.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "selinv.hpp"

namespace gmrf {

// part[p][c] = sum over the rows [c len_n, (c + 1) len_n) of d_i (Q d)_i  +  noise * sum over [c len_m, (c + 1) len_m) of o_k^2
// with d = x_prior - x.  Q is symmetric, so the CSC arrays of its pattern are read as CSR.  The partition depends on n and m
// only, thread t takes the rows t, t + 256, ... of its chunk in order and the workgroup adds its 256 sums in a fixed tree:
// no atomics, and a problem's value does not depend on the batch it sits in (pattern_dot_part / pattern_dot_sum do the same).
__global__ __launch_bounds__(256) void gn_objective_part(const int64_t* __restrict__ qptr, const int32_t* __restrict__ qrow,
                                                         const double* __restrict__ q, int64_t q_stride,
                                                         const double* __restrict__ xp, const double* __restrict__ x, int64_t n,
                                                         const double* __restrict__ o, int64_t m, double noise, int64_t len_n,
                                                         int64_t len_m, double* __restrict__ part) {
    __shared__ double red[256];
    const int64_t c = blockIdx.x, p = blockIdx.y, nch = gridDim.x;
    q += p * q_stride; xp += p * n; x += p * n; o += p * m;
    double acc = 0.0;
    const int64_t i1 = min(n, (c + 1) * len_n);
    for (int64_t i = c * len_n + threadIdx.x; i < i1; i += 256) {
        double s = 0.0;
        for (int64_t e = qptr[i]; e < qptr[i + 1]; ++e) {
            const int32_t r = qrow[e];
            s = fma(q[e], xp[r] - x[r], s);
        }
        acc = fma(xp[i] - x[i], s, acc);
    }
    double acc_o = 0.0;
    const int64_t k1 = min(m, (c + 1) * len_m);
    for (int64_t k = c * len_m + threadIdx.x; k < k1; k += 256) acc_o = fma(o[k], o[k], acc_o);
    const double v = block_sum_256(fma(noise, acc_o, acc), red);
    if (threadIdx.x == 0) part[p * nch + c] = v;
}

// o[p][k] = y[p][k] - f[p][k]   (y == nullptr: zero observations, as the Burgers scripts have them)
__global__ __launch_bounds__(256) void gn_obs_diff(const double* __restrict__ y, const double* __restrict__ f, int64_t m,
                                                   double* __restrict__ o) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const int64_t at = (int64_t)blockIdx.y * m + k;
    o[at] = (y ? y[at] : 0.0) - f[at];
}

struct GnState {
    double* last;           // [B] objective before the last step taken (+Inf at the start)
    double* cur;            // [B] objective at x
    int32_t* steps;         // [B] steps taken
    int32_t* active;        // [B] 1 while rel_diff(last, cur) > rtol and steps < max_steps
    int32_t* take;          // [B] 1: this iteration's candidate becomes the problem's x (gn_apply)
    double* hist;           // [B][max_steps + 1] objective history, hist[p][0] at the start point
    unsigned* host_active;  // mapped host word: how many problems are still active
};

// The stop rule, one thread per problem.  init: obj is the objective at the start point.  Else obj is the objective at the
// candidate of this iteration: an active problem takes it (last <- cur <- obj, the step is counted, the history grows) and is
// tested again; a problem that has stopped is frozen -- none of its words change.  One workgroup: thread 0 counts at the end.
__global__ __launch_bounds__(256) void gn_decide(GnState s, const double* __restrict__ obj, int64_t B, double rtol,
                                                 int32_t max_steps, int32_t init) {
    for (int64_t p = threadIdx.x; p < B; p += 256) {
        int32_t take = 0;
        if (init) {
            s.last[p] = INFINITY; s.cur[p] = obj[p]; s.steps[p] = 0;
            s.hist[p * (max_steps + 1)] = obj[p];
            take = 1;
        } else if (s.active[p]) {
            s.last[p] = s.cur[p]; s.cur[p] = obj[p]; s.steps[p] += 1;
            s.hist[p * (max_steps + 1) + s.steps[p]] = obj[p];
            take = 1;
        }
        if (take) {
            const double last = s.last[p], cur = s.cur[p];
            s.active[p] = (fabs(last - cur) / fabs(cur) > rtol && s.steps[p] < max_steps) ? 1 : 0;
        }
        s.take[p] = init ? 0 : take;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned cnt = 0;
        for (int64_t p = 0; p < B; ++p) cnt += s.active[p] ? 1u : 0u;
        *reinterpret_cast<volatile unsigned*>(s.host_active) = cnt;
    }
}

// x[p] <- xn[p], obs_diff[p] <- on[p] for the problems that took this iteration's candidate
__global__ __launch_bounds__(256) void gn_apply(const int32_t* __restrict__ take, const double* __restrict__ xn, double* __restrict__ x,
                                                int64_t n, const double* __restrict__ on, double* __restrict__ o, int64_t m) {
    const int64_t p = blockIdx.y;
    if (!take[p]) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[p * n + i] = xn[p * n + i];
    if (i < m) o[p * m + i] = on[p * m + i];
}

}  // namespace gmrf
