// FEM fields evaluated at arbitrary points of the mesh (gmrf_eval_*, gmrf_hip.hip): pred = E f with E the reference's
// evaluation_matrix(disc, pred_coords), and the error metrics of pred against a truth in the same pass.
// The table of E is built once on the host in double precision (field_eval_line_row / field_eval_tri_row below) and uploaded as
// idx [W][npts] (32-bit) and w [W][npts], W = 2 (P1 line), 3 (quadratic line, P1 triangle) or 6 (quadratic triangle) entries per
// point in ascending dof index.  One thread per (field row, point), consecutive threads on consecutive points: the table loads
// coalesce, the W reads of the field row are the only irregular access.  ONE rounding sequence for every result,
//     pred = w0 f[idx0];  pred = fma(wk, f[idxk], pred), k = 1 .. W - 1,
// so a point's value is the same bits in every batch, for every number of rows and on every call.  No atomics, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "burgers_prior.hpp"        // block_sum_256 (selinv.hpp), block_max_256

namespace gmrf {

// ------------------------------------------------------------------------------------------------ geometry (host, once)
// Sorts the W entries of a row by dof index (insertion sort: W <= 6, the indices of a row are distinct).
inline void field_eval_sort_row(int W, int64_t* idx, double* w) {
    for (int a = 1; a < W; ++a)
        for (int b = a; b > 0 && idx[b - 1] > idx[b]; --b) { std::swap(idx[b - 1], idx[b]); std::swap(w[b - 1], w[b]); }
}

// Point x of the line of nc cells of length h with ns dofs numbered by position (periodic: the last cell's right dof is dof 0).
inline void field_eval_line_row(int order, int64_t nc, int64_t ns, double h, double x, int64_t* idx, double* w) {
#pragma clang fp contract(off)
    const int64_t e = std::min((int64_t)std::floor(x / h), nc - 1);
    const double xi = std::min(1.0, std::max(-1.0, 2.0 * (x - (double)e * h) / h - 1.0));
    if (order == 1) {
        idx[0] = e; idx[1] = (e + 1) % ns;
        w[0] = (1.0 - xi) / 2.0; w[1] = (1.0 + xi) / 2.0;
    } else {
        idx[0] = 2 * e; idx[1] = (2 * e + 2) % ns; idx[2] = 2 * e + 1;
        w[0] = 0.5 * xi * (xi - 1.0); w[1] = 0.5 * xi * (xi + 1.0); w[2] = 1.0 - xi * xi;
    }
    field_eval_sort_row(order + 1, idx, w);
}

// Point (x, y) of the unit square's nx x ny vertex mesh, quads cut by the diagonal n00 - n11; t <= s is the lower triangle.
inline void field_eval_tri_row(int order, int64_t nx, int64_t ny, double x, double y, int64_t* idx, double* w) {
#pragma clang fp contract(off)
    const double hx = 1.0 / (double)(nx - 1), hy = 1.0 / (double)(ny - 1);
    const int64_t qx = std::min((int64_t)std::floor(x / hx), nx - 2), qy = std::min((int64_t)std::floor(y / hy), ny - 2);
    const double s = std::min(1.0, std::max(0.0, (x - (double)qx * hx) / hx));
    const double t = std::min(1.0, std::max(0.0, (y - (double)qy * hy) / hy));
    const bool lower = t <= s;
    // vertices (i, j) of the cell in its local order and their barycentrics
    const int64_t vi[3] = {qx, qx + 1, lower ? qx + 1 : qx}, vj[3] = {qy, lower ? qy : qy + 1, qy + 1};
    const double lam[3] = {lower ? 1.0 - s : 1.0 - t, lower ? s - t : s, lower ? t : t - s};
    if (order == 1) {
        for (int k = 0; k < 3; ++k) { idx[k] = vi[k] + nx * vj[k]; w[k] = lam[k]; }
    } else {
        const int64_t lx = 2 * nx - 1;
        for (int k = 0; k < 3; ++k) {
            const int a = k, b = (k + 1) % 3;
            idx[k] = 2 * vi[k] + lx * (2 * vj[k]);
            w[k] = lam[k] * (2.0 * lam[k] - 1.0);
            idx[3 + k] = (vi[a] + vi[b]) + lx * (vj[a] + vj[b]);
            w[3 + k] = 4.0 * lam[a] * lam[b];
        }
    }
    field_eval_sort_row(order == 1 ? 3 : 6, idx, w);
}

// ------------------------------------------------------------------------------------------------ kernels
// Point c of the field row f: the one rounding sequence.
template <int W>
__device__ __forceinline__ double field_eval_point(const int32_t* __restrict__ idx, const double* __restrict__ w, int64_t npts,
                                                   int64_t c, const double* __restrict__ f) {
    double acc = w[c] * f[idx[c]];
#pragma unroll
    for (int k = 1; k < W; ++k) acc = fma(w[k * npts + c], f[idx[k * npts + c]], acc);
    return acc;
}

// pred[r][c] for the rows r = blockIdx.y, blockIdx.y + gridDim.y, ... < rows: grid = (ceil(npts / 256), min(rows, 65535)).  A
// thread keeps its point's W entries in registers over its rows.
template <int W>
__global__ __launch_bounds__(256) void field_eval_apply(const int32_t* __restrict__ idx, const double* __restrict__ w, int64_t npts,
                                                        int64_t ns, int64_t rows, const double* __restrict__ fields,
                                                        double* __restrict__ pred) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= npts) return;
    int32_t j[W];
    double a[W];
#pragma unroll
    for (int k = 0; k < W; ++k) { j[k] = idx[k * npts + c]; a[k] = w[k * npts + c]; }
    for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
        const double* f = fields + r * ns;
        double acc = a[0] * f[j[0]];
#pragma unroll
        for (int k = 1; k < W; ++k) acc = fma(a[k], f[j[k]], acc);
        pred[r * npts + c] = acc;
    }
}

// field_errors_part (burgers_prior.hpp) with pred formed as it is read: problem p's nt field rows [nt][ns] against truth
// [nt npts], elements [first, nt npts).  Same partition (workgroup (c, p) takes [first + c len, first + (c + 1) len), thread t its
// elements t, t + 256, ... in order), same accumulation and the same LDS trees, so part -- and field_errors_finish's result -- is
// bitwise that of field_eval_apply followed by field_errors_part.  grid = (nch, batch).
template <int W>
__global__ __launch_bounds__(256) void field_eval_errors_part(const int32_t* __restrict__ idx, const double* __restrict__ w,
                                                              int64_t npts, int64_t ns, int64_t nt,
                                                              const double* __restrict__ fields, const double* __restrict__ truth,
                                                              int64_t first, int64_t len, double* __restrict__ part) {
    __shared__ double red[256];
    const int64_t c = blockIdx.x, p = blockIdx.y, nch = gridDim.x, n = nt * npts;
    fields += p * nt * ns; truth += p * n;
    double acc_d = 0.0, acc_s = 0.0, mx = 0.0;
    const int64_t i0 = first + c * len + threadIdx.x, i1 = min(n, first + (c + 1) * len);
    // (slice, pt) of element i, stepped by 256 = dq npts + dr without a division per element
    const int64_t dq = 256 / npts, dr = 256 % npts;
    int64_t slice = i0 / npts, pt = i0 % npts;
    for (int64_t i = i0; i < i1; i += 256) {
        const double s = truth[i], d = field_eval_point<W>(idx, w, npts, pt, fields + slice * ns) - s;
        acc_d = fma(d, d, acc_d);
        acc_s = fma(s, s, acc_s);
        mx = fmax(mx, fabs(d));
        slice += dq; pt += dr;
        if (pt >= npts) { pt -= npts; ++slice; }
    }
    const double sd = block_sum_256(acc_d, red);
    __syncthreads();
    const double ss = block_sum_256(acc_s, red);
    const double m = block_max_256(mx, red);
    if (threadIdx.x == 0) {
        double* o = part + (p * nch + c) * 3;
        o[0] = sd; o[1] = ss; o[2] = m;
    }
}

}  // namespace gmrf
