// FEM fields evaluated at arbitrary points of the mesh (gmrf_eval_*, gmrf_hip.hip): pred = E f with E the reference's
// evaluation_matrix(disc, pred_coords), and the error metrics of pred against a truth in the same pass.
// The table of E is built once on the host in double precision (field_eval_line_row / field_eval_tri_row below) and uploaded as
// idx [W][npts] (32-bit) and w [W][npts], W = 2 (P1 line), 3 (quadratic line, P1 triangle) or 6 (quadratic triangle) entries per
// point in ascending dof index.  One thread per (field row, point), consecutive threads on consecutive points: the table loads
// coalesce, the W reads of the field row are the only irregular access.  ONE rounding sequence for every result,
//     pred = w0 f[idx0];  pred = fma(wk, f[idxk], pred), k = 1 .. W - 1,
// so a point's value is the same bits in every batch, for every number of rows and on every call.  No atomics, no scratch.
// The pointwise predictive variance diag(E Sigma E^T) and the calibration of pred under it follow the same scheme over the selected
// inverse on the pair pattern (field_eval_pairs, field_eval_var, field_eval_calibration_part at the end of this file).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

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

// Pair table of the rows idx [npts][W] (ascending within a row) over ns dofs: the pattern P (ns x ns, symmetric, both triangles,
// sorted CSR) of exactly the dof pairs that some point uses -- the diagonal of every dof used among them -- and, for point c and
// pair (a >= b) at k = a (a + 1) / 2 + b, the position pos[k npts + c] of the entry (idx_a, idx_b) of the lower triangle in P's CSR
// order.  False if P has 2^31 entries or more (positions are 32-bit).
inline bool field_eval_pairs(int W, int64_t npts, int64_t ns, const int64_t* idx, std::vector<int64_t>& rowptr,
                             std::vector<int64_t>& colidx, std::vector<int32_t>& pos) {
    std::vector<int64_t> keys;                          // row ns + column, both triangles
    keys.reserve((size_t)(npts * W * W));
    for (int64_t c = 0; c < npts; ++c) {
        const int64_t* r = idx + c * W;
        for (int a = 0; a < W; ++a)
            for (int b = 0; b < W; ++b) keys.push_back(r[a] * ns + r[b]);
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    if (keys.size() >= ((size_t)1 << 31)) return false;
    rowptr.assign((size_t)ns + 1, 0);
    colidx.resize(keys.size());
    for (size_t e = 0; e < keys.size(); ++e) { rowptr[(size_t)(keys[e] / ns) + 1]++; colidx[e] = keys[e] % ns; }
    for (int64_t r = 0; r < ns; ++r) rowptr[(size_t)r + 1] += rowptr[(size_t)r];
    pos.resize((size_t)(npts * (W * (W + 1) / 2)));
    for (int64_t c = 0; c < npts; ++c) {
        const int64_t* r = idx + c * W;
        for (int a = 0, k = 0; a < W; ++a)
            for (int b = 0; b <= a; ++b, ++k)
                pos[(size_t)(k * npts + c)] = (int32_t)(std::lower_bound(keys.begin(), keys.end(), r[a] * ns + r[b]) - keys.begin());
    }
    return true;
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

// ------------------------------------------------------------------------------------------------ pointwise predictive variance
// var = diag(E Sigma E^T) at the points: row c of E has W dofs i_0 < ... < i_{W-1} in one element, so
//     v_c = sum_ab w_a w_b Sigma[i_a, i_b]
// over W (W + 1) / 2 distinct entries of Sigma.  The pair table (field_eval_pairs below, built on the host at creation) holds the
// spatial pattern P of those entries and, per point and pair (a >= b) at k = a (a + 1) / 2 + b, the position pos[k][c] of
// (i_a, i_b) in P's CSR order; slice t of a space-time field reads I_nt (x) P at t nnz(P) + pos.  sig is the selected inverse on
// that pattern (gmrf_bt_selinv), [problems][nt nnz(P)].  ONE rounding sequence,
//     s_a = w_0 Sigma[a,0];  s_a = fma(w_b, Sigma[a,b], s_a), b = 1 .. W - 1;   v = w_0 s_0;  v = fma(w_a, s_a, v), a = 1 .. W - 1,
// so a point's variance is the same bits in every batch and on every call.  No atomics, no scratch.
__host__ __device__ constexpr int field_eval_pair(int a, int b) { return a >= b ? a * (a + 1) / 2 + b : b * (b + 1) / 2 + a; }

// var[r][c] for the rows r = (problem, slice) = blockIdx.y, blockIdx.y + gridDim.y, ... < problems nt: grid as field_eval_apply.  A
// thread keeps its point's weights and positions in registers over its rows; the W (W + 1) / 2 reads of sig are the only
// irregular access.
template <int W>
__global__ __launch_bounds__(256) void field_eval_var(const int32_t* __restrict__ pos, const double* __restrict__ w, int64_t npts,
                                                      int64_t nnzp, int64_t rows, const double* __restrict__ sig,
                                                      double* __restrict__ var) {
    constexpr int NP = W * (W + 1) / 2;
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= npts) return;
    int32_t q[NP];
    double a[W];
#pragma unroll
    for (int k = 0; k < NP; ++k) q[k] = pos[k * npts + c];
#pragma unroll
    for (int k = 0; k < W; ++k) a[k] = w[k * npts + c];
    for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
        const double* s = sig + r * nnzp;       // row r = p nt + t: problem p's slice t starts at p (nt nnzp) + t nnzp
        double e[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) e[k] = s[q[k]];
        double v = 0.0;
#pragma unroll
        for (int i = 0; i < W; ++i) {
            double si = a[0] * e[field_eval_pair(i, 0)];
#pragma unroll
            for (int j = 1; j < W; ++j) si = fma(a[j], e[field_eval_pair(i, j)], si);
            v = i == 0 ? a[0] * si : fma(a[i], si, v);
        }
        var[r * npts + c] = v;
    }
}

// Calibration of a prediction against a truth under those variances, problem p's nt field rows [nt][ns], truth and var
// [nt npts], elements [first, nt npts): z = (pred - truth) / sqrt(v), pred formed as field_eval_errors_part forms it.  The
// partition and the LDS trees are field_eval_errors_part's: part[p][c][4] = (sum z^2, #{|z| <= zcrit}, sum -(log(2 pi v) + z^2) / 2,
// min v).  The count is an integer per thread and is summed as a double, which is exact below 2^53.  grid = (nch, batch).
template <int W>
__global__ __launch_bounds__(256) void field_eval_calibration_part(const int32_t* __restrict__ idx, const double* __restrict__ w,
                                                                   int64_t npts, int64_t ns, int64_t nt,
                                                                   const double* __restrict__ fields,
                                                                   const double* __restrict__ truth, const double* __restrict__ var,
                                                                   double zcrit, int64_t first, int64_t len,
                                                                   double* __restrict__ part) {
    __shared__ double red[256];
    const int64_t c = blockIdx.x, p = blockIdx.y, nch = gridDim.x, n = nt * npts;
    fields += p * nt * ns; truth += p * n; var += p * n;
    double acc_z = 0.0, acc_l = 0.0, mn = __builtin_huge_val();
    int cnt = 0;
    const int64_t i0 = first + c * len + threadIdx.x, i1 = min(n, first + (c + 1) * len);
    const int64_t dq = 256 / npts, dr = 256 % npts;
    int64_t slice = i0 / npts, pt = i0 % npts;
    for (int64_t i = i0; i < i1; i += 256) {
        const double v = var[i], z = (field_eval_point<W>(idx, w, npts, pt, fields + slice * ns) - truth[i]) / sqrt(v);
        acc_z = fma(z, z, acc_z);
        cnt += fabs(z) <= zcrit ? 1 : 0;
        acc_l += -0.5 * fma(z, z, log(6.283185307179586 * v));
        mn = fmin(mn, v);
        slice += dq; pt += dr;
        if (pt >= npts) { pt -= npts; ++slice; }
    }
    const double sz = block_sum_256(acc_z, red);
    __syncthreads();
    const double sc = block_sum_256((double)cnt, red);
    __syncthreads();
    const double sl = block_sum_256(acc_l, red);
    const double m = -block_max_256(-mn, red);
    if (threadIdx.x == 0) {
        double* o = part + (p * nch + c) * 4;
        o[0] = sz; o[1] = sc; o[2] = sl; o[3] = m;
    }
}

// out[p] = (mean z^2, coverage, mean log predictive density, min variance) from a problem's nch chunks, summed as
// field_errors_finish sums its own.
__global__ __launch_bounds__(256) void field_eval_calibration_finish(const double* __restrict__ part, int64_t nch, int64_t count,
                                                                     double* __restrict__ out) {
    __shared__ double red[256];
    const int64_t p = blockIdx.y;
    const double* q = part + p * nch * 4;
    double acc_z = 0.0, acc_c = 0.0, acc_l = 0.0, mn = __builtin_huge_val();
    for (int64_t c = threadIdx.x; c < nch; c += 256) {
        acc_z += q[4 * c]; acc_c += q[4 * c + 1]; acc_l += q[4 * c + 2]; mn = fmin(mn, q[4 * c + 3]);
    }
    const double sz = block_sum_256(acc_z, red);
    __syncthreads();
    const double sc = block_sum_256(acc_c, red);
    __syncthreads();
    const double sl = block_sum_256(acc_l, red);
    const double m = -block_max_256(-mn, red);
    if (threadIdx.x == 0) {
        out[4 * p] = sz / (double)count;
        out[4 * p + 1] = sc / (double)count;
        out[4 * p + 2] = sl / (double)count;
        out[4 * p + 3] = m;
    }
}

}  // namespace gmrf
