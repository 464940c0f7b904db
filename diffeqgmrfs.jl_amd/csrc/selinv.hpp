// Selected inverse on a sparsity pattern (gmrf_bt_selinv / gmrf_bt_trace_inv, gmrf_hip.hip: selinv_pattern).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gmrf {

// One block step of the pattern recurrence: entries [e0, e0 + ne) of the plan; the first nd read the diagonal block
// Sd (its lower triangle, row-major), the others the coupling block Sc.  src[e]: element offset inside the block,
// slot[e] / slot2[e]: where the value goes in the problem's [nnz] output (slot2 < 0: one place only).
// grid = (ceil(ne / 256), problems); pS: per-problem stride of Sd and Sc, pout: of out.
__global__ __launch_bounds__(256) void selinv_scatter(const double* __restrict__ Sd, const double* __restrict__ Sc, int64_t pS,
                                                      const int64_t* __restrict__ src, const int64_t* __restrict__ slot,
                                                      const int64_t* __restrict__ slot2, int64_t e0, int64_t nd, int64_t ne,
                                                      double* __restrict__ out, int64_t pout) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= ne) return;
    const int64_t e = e0 + k;
    const int64_t p = blockIdx.y;
    const double v = (k < nd ? Sd : Sc)[p * pS + src[e]];
    double* o = out + p * pout;
    o[slot[e]] = v;
    const int64_t s2 = slot2[e];
    if (s2 >= 0) o[s2] = v;
}

// out[p][j] = sum_e sig[p][e] * dv[p][j][e] in two launches over a fixed partition of the entries (it depends on nnz only), no
// atomics: the same inputs give the same bits.  pattern_dot_part: workgroup (c, j, p) sums the entries [c len, (c + 1) len) --
// thread t takes t, t + 256, ... in order, then a fixed-shape tree in LDS -- into part[p][j][c]; pattern_dot_sum: workgroup
// (j, p) = (blockIdx.x, blockIdx.y) adds the nch partial sums the same way.
__device__ inline double block_sum_256(double v, double* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(256) void pattern_dot_part(const double* __restrict__ sig, const double* __restrict__ dv, int64_t nnz,
                                                        int64_t m, int64_t len, double* __restrict__ part) {
    __shared__ double red[256];
    const int64_t c = blockIdx.x, j = blockIdx.y, p = blockIdx.z, nch = gridDim.x;
    const double* s = sig + p * nnz;
    const double* d = dv + (p * m + j) * nnz;
    const int64_t e1 = min(nnz, (c + 1) * len);
    double acc = 0.0;
    for (int64_t e = c * len + threadIdx.x; e < e1; e += 256) acc = fma(s[e], d[e], acc);
    const double v = block_sum_256(acc, red);
    if (threadIdx.x == 0) part[(p * m + j) * nch + c] = v;
}

__global__ __launch_bounds__(256) void pattern_dot_sum(const double* __restrict__ part, int64_t nch, int64_t m, double* __restrict__ out) {
    __shared__ double red[256];
    const int64_t j = blockIdx.x, p = blockIdx.y;
    const double* q = part + (p * m + j) * nch;
    double acc = 0.0;
    for (int64_t c = threadIdx.x; c < nch; c += 256) acc += q[c];
    const double v = block_sum_256(acc, red);
    if (threadIdx.x == 0) out[p * m + j] = v;
}

}  // namespace gmrf
