// The prior of the Burgers space-time GMRF for a batch of problems on the device: the "Prior" stage of the data-set loop
// (form_prior, scripts/burgers/solve_burgers_gmrf-fem.jl:86-107) and the right-hand side of its "Initial condition" stage
// (condition_on_observations(x, A_ic, ic_noise, ic), :161), as `workloads.burgers(ns, nt, ic_noise, 0.0, ic)` states them on the
// periodic P1 line with lumped mass, time-major index t ns + s:
//     Q_ic = Q_prior + ic_noise A_ic' A_ic,        rhs = Q_prior (bulk 1) + ic_noise A_ic' ic,        bulk = mean(ic).
// On the uniform mesh every block is a circulant stencil, and a problem enters only through gamma = -c bulk:
//     G = M + dt (nu c S + gamma Adv) = circ(gm, g0, gp),   W = w I,   w = 1 / (dt tau^2 h),   M = h I
//     diagonal block t > 0:  w G'G (+ w h^2 I for t < nt-1)      offsets 0, +-1, +-2
//     diagonal block 0:      Q0 = K M^-1 K, K = kappa^2 M + S (+ w h^2 I) + ic_noise I
//     block (t, t-1):        -w h G'   (and its transpose above the diagonal)      offsets 0, +-1
// The pattern is structural -- fixed by (ns, nt), an entry that happens to be 0.0 is stored -- symmetric CSC, both triangles,
// rows ascending: column (t, i) holds {i-1, i, i+1} of slice t-1, {i-2 .. i+2} of slice t, {i-1, i, i+1} of slice t+1 (periodic;
// ns >= 5 keeps the offsets apart).  All arrays are problem-major; blockIdx.y is the problem.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "selinv.hpp"

namespace gmrf {

struct BurgersPriorArgs {
    int64_t ns, nt;
    double dt, nu, ic_noise;
};

inline int64_t burgers_prior_nnz(int64_t ns, int64_t nt) { return (11 * nt - 6) * ns; }

// first entry of column (t, i): the columns of the first and the last slice hold 8 entries, the others 11
__host__ __device__ inline int64_t burgers_prior_colptr(int64_t ns, int64_t nt, int64_t t, int64_t i) {
    if (t == 0) return 8 * i;
    if (t < nt - 1) return 8 * ns + (t - 1) * 11 * ns + 11 * i;
    return 8 * ns + (nt - 2) * 11 * ns + 8 * i;
}

// (row, column) of stored entry e: the one statement of the pattern, for the host's CSC arrays and the value kernel alike
__host__ __device__ inline void burgers_prior_entry(int64_t ns, int64_t nt, int64_t e, int64_t* row, int64_t* col) {
    int64_t t, i, k;
    const int64_t first = 8 * ns, mid = (nt - 2) * 11 * ns;
    if (e < first) { t = 0; i = e / 8; k = e % 8; }
    else if (e < first + mid) { const int64_t r = e - first; t = 1 + r / (11 * ns); i = (r % (11 * ns)) / 11; k = (r % (11 * ns)) % 11; }
    else { const int64_t r = e - first - mid; t = nt - 1; i = r / 8; k = r % 8; }
    int64_t blk, wd;                    // block row of the entry, half width of its stencil
    if (t > 0 && k < 3) { blk = t - 1; wd = 1; }
    else {
        if (t > 0) k -= 3;
        if (k < 5) { blk = t; wd = 2; }
        else { k -= 5; blk = t + 1; wd = 1; }
    }
    // the k-th smallest of the rows (i + o) mod ns, o = -wd .. wd
    int64_t r_k = 0;
    for (int64_t o = -wd; o <= wd; ++o) {
        const int64_t r = (i + o + ns) % ns;
        int64_t rank = 0;
        for (int64_t o2 = -wd; o2 <= wd; ++o2) rank += ((i + o2 + ns) % ns < r) ? 1 : 0;
        if (rank == k) r_k = r;
    }
    *row = blk * ns + r_k;
    *col = t * ns + i;
}

// The stencil coefficients of one problem, by |offset|: d0 the first diagonal block (Q0), dg the other diagonal blocks (w G'G),
// lo the blocks beside the diagonal by (index in the later slice) - (index in the earlier slice) = 0, +1, -1; wh2 = w h^2.  The
// scalar constants are written as workloads.burgers writes them.
struct BurgersPriorCoef {
    double d0[3], dg[3], lo[3], wh2;
};

__host__ __device__ inline BurgersPriorCoef burgers_prior_coef(const BurgersPriorArgs& a, double bulk) {
    const double h = 1.0 / (double)a.ns;
    const double c = 1.0 / a.nu, nuc = a.nu * c, gamma = -c * bulk, tau = 0.1 * sqrt(c), kappa2 = 12.0 * (double)a.ns;
    const double w = (1.0 / (a.dt * tau * tau)) / h;
    const double g0 = h + a.dt * (nuc * (2.0 / h)), gp = a.dt * (nuc * (-1.0 / h) + gamma * 0.5), gm = a.dt * (nuc * (-1.0 / h) + gamma * -0.5);
    const double k0 = kappa2 * h + 2.0 / h, k1 = -1.0 / h, ih = 1.0 / h, wh = w * h;
    BurgersPriorCoef k;
    k.d0[0] = (k0 * k0 + k1 * k1 + k1 * k1) * ih; k.d0[1] = (k0 * k1 + k1 * k0) * ih; k.d0[2] = (k1 * k1) * ih;
    k.dg[0] = w * (g0 * g0 + gp * gp + gm * gm);  k.dg[1] = w * (g0 * gp + gm * g0);  k.dg[2] = w * (gm * gp);
    k.lo[0] = -(wh * g0); k.lo[1] = -(wh * gp); k.lo[2] = -(wh * gm);
    k.wh2 = wh * h;
    return k;
}

// entry (row, col) of Q_ic.  (row, col) and (col, row) take the same path with the same arguments: the values are bitwise symmetric.
__host__ __device__ inline double burgers_prior_value(const BurgersPriorArgs& a, const BurgersPriorCoef& k, int64_t row, int64_t col) {
    const int64_t ns = a.ns, tr = row / ns, ia = row % ns, tc = col / ns, ib = col % ns;
    if (tr == tc) {
        const int64_t d = (ia - ib + ns) % ns;
        const int cls = d == 0 ? 0 : ((d == 1 || d == ns - 1) ? 1 : 2);
        double v = tr == 0 ? k.d0[cls] : k.dg[cls];
        if (cls == 0) {
            if (tr < a.nt - 1) v += k.wh2;
            if (tr == 0) v += a.ic_noise;
        }
        return v;
    }
    const int64_t d = tr > tc ? (ia - ib + ns) % ns : (ib - ia + ns) % ns;      // later slice's index - earlier slice's
    return k.lo[d == 0 ? 0 : (d == 1 ? 1 : 2)];
}

// bulk[p] = mean(ic[p]): one workgroup per problem, thread t adds the nodes t, t + 256, ... in order, then the fixed tree.
__global__ __launch_bounds__(256) void burgers_bulk_batch(const double* __restrict__ ic, int64_t ns, double* __restrict__ bulk) {
    __shared__ double red[256];
    const int64_t p = blockIdx.y;
    ic += p * ns;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < ns; i += 256) acc += ic[i];
    const double sum = block_sum_256(acc, red);
    if (threadIdx.x == 0) bulk[p] = sum / (double)ns;
}

// q[p][e]: one thread per stored entry
__global__ __launch_bounds__(256) void burgers_prior_values_batch(BurgersPriorArgs a, const double* __restrict__ bulk, int64_t nnz,
                                                                  double* __restrict__ q) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    const int64_t p = blockIdx.y;
    const BurgersPriorCoef k = burgers_prior_coef(a, bulk[p]);
    int64_t row, col;
    burgers_prior_entry(a.ns, a.nt, e, &row, &col);
    q[p * nnz + e] = burgers_prior_value(a, k, row, col);
}

// qx[p][r] = (row r of Q_prior) 1 bulk_p + ic_noise [ic_p; 0]_r: the row's stencil coefficients added in the fixed order
// slice t-1 (offsets 0, +1, -1), slice t (-2, -1, 0, +1, +2), slice t+1 (0, +1, -1); Q_prior is Q_ic without the ic_noise term.
__global__ __launch_bounds__(256) void burgers_prior_rhs_batch(BurgersPriorArgs a, const double* __restrict__ bulk,
                                                               const double* __restrict__ ic, double* __restrict__ qx) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, n = a.ns * a.nt;
    if (r >= n) return;
    const int64_t p = blockIdx.y, t = r / a.ns;
    const double b = bulk[p];
    const BurgersPriorCoef k = burgers_prior_coef(a, b);
    const double* dd = t == 0 ? k.d0 : k.dg;
    const double beside = k.lo[0] + k.lo[1] + k.lo[2];
    double s = 0.0;
    if (t > 0) s += beside;
    s += dd[2]; s += dd[1]; s += (t < a.nt - 1 ? dd[0] + k.wh2 : dd[0]); s += dd[1]; s += dd[2];
    if (t < a.nt - 1) s += beside;
    double v = s * b;
    if (t == 0) v += a.ic_noise * ic[p * a.ns + r];
    qx[p * n + r] = v;
}

// ------------------------------------------------------------------------------------------------
// Error metrics of a batch of fields against their truths (src/metrics.jl:3-13) over the elements [first, n) of every problem:
//     out[p] = (rel_err, rmse, max_err) = (|d| / |soln|, sqrt(mean(d^2)), max |d|),   d = pred - soln.
// field_errors_part: workgroup (c, p) takes the elements [first + c len, first + (c + 1) len), thread t the elements t, t + 256, ...
// of them in order, then fixed trees in LDS -> part[p][c][3] = (sum d^2, sum soln^2, max |d|); field_errors_finish adds / compares
// a problem's chunks the same way.  The partition depends on (n, first) only: no atomics, the same bits on every call and in
// every batch.
__device__ inline double block_max_256(double v, double* red) {
    const int t = threadIdx.x;
    __syncthreads();                    // (red may still be read by a sum before)
    red[t] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) red[t] = fmax(red[t], red[t + w]);
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(256) void field_errors_part(const double* __restrict__ pred, const double* __restrict__ soln, int64_t n,
                                                         int64_t first, int64_t len, double* __restrict__ part) {
    __shared__ double red[256];
    const int64_t c = blockIdx.x, p = blockIdx.y, nch = gridDim.x;
    pred += p * n; soln += p * n;
    double acc_d = 0.0, acc_s = 0.0, mx = 0.0;
    const int64_t i1 = min(n, first + (c + 1) * len);
    for (int64_t i = first + c * len + threadIdx.x; i < i1; i += 256) {
        const double s = soln[i], d = pred[i] - s;
        acc_d = fma(d, d, acc_d);
        acc_s = fma(s, s, acc_s);
        mx = fmax(mx, fabs(d));
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

__global__ __launch_bounds__(256) void field_errors_finish(const double* __restrict__ part, int64_t nch, int64_t count,
                                                           double* __restrict__ out) {
    __shared__ double red[256];
    const int64_t p = blockIdx.y;
    const double* q = part + p * nch * 3;
    double acc_d = 0.0, acc_s = 0.0, mx = 0.0;
    for (int64_t c = threadIdx.x; c < nch; c += 256) { acc_d += q[3 * c]; acc_s += q[3 * c + 1]; mx = fmax(mx, q[3 * c + 2]); }
    const double sd = block_sum_256(acc_d, red);
    __syncthreads();
    const double ss = block_sum_256(acc_s, red);
    const double m = block_max_256(mx, red);
    if (threadIdx.x == 0) {
        out[3 * p] = sqrt(sd) / sqrt(ss);
        out[3 * p + 1] = sqrt(sd / (double)count);
        out[3 * p + 2] = m;
    }
}

}  // namespace gmrf
