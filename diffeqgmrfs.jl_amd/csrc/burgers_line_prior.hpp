// The prior of burgers_prior.hpp on every line the tangent serves (burgers_line.hpp): order 1 or 2, the periodic line or the
// interval with pinned ends, any length -- the lines of the reference's two Burgers scripts (scripts/burgers/solve_burgers_gmrf-fem.jl:
// 71-72 runs form_prior, :86-107, on the periodic QUADRATIC line; _research/burgers_chen24.jl on the quadratic Dirichlet interval),
// as `workloads.burgers_line_prior_from_bulk` states it: with l the lumped mass (row sums of the consistent mass), S the stiffness,
// Adv[i][j] = int phi_i phi_j', time-major index t ns + s and c = 1 / nu, gamma = -c bulk, tau = 0.1 sqrt(c), kappa^2 = 12 nc,
//     K = kappa^2 diag(l) + S,   G = diag(l) + dt (nu c S + gamma Adv),   w_k = (1 / (dt tau^2)) / l_k
//     diagonal block t > 0:  G' W G (+ diag(l w l) for t < nt-1)        offsets 0 .. +-2 order
//     diagonal block 0:      K diag(1 / l) K (+ diag(l w l)) + ic_noise on the observed dofs
//     block (t, t-1):        -G' W diag(l)   (and its transpose above the diagonal)        offsets 0 .. +-order
//     dirichlet:             + pin on the diagonal of dofs 0 and ns-1 of every slice
//     bulk = mean of ic over the observed dofs,   rhs = Q_prior(without pins) (bulk 1) + ic_noise [ic at the observed dofs; 0].
// The mesh is uniform but, unlike the P1 periodic line, not every row is the same: a quadratic vertex couples five dofs, a midpoint
// three, and the ends of the interval are clipped.  So nothing is tabulated: an entry of S, Adv or l comes from the element matrices
// on the fly, from the dof's parity and its distance to an end (line_prior_sa, line_prior_lumped), and an entry of Q is the sum over
// the at most 2 order + 1 rows k that both of its dofs couple to, k ascending.
// The pattern is structural, symmetric CSC with both triangles and rows ascending; periodic offsets wrap (order nc >= 4 order + 1
// keeps them apart), dirichlet offsets are clipped to the slice.  All arrays are problem-major; blockIdx.y is the problem.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "selinv.hpp"

namespace gmrf {

struct BurgersLinePriorArgs {
    int64_t ns, nt, nc;
    int order, periodic, vertices;      // vertices: the initial condition is observed at the even dofs only (order 2)
    double dt, nu, ic_noise, h, pin;    // h: cell length
};

// ------------------------------------------------------------------------------------------------ pattern
// rows of a slice that column i holds at half width R: all 2R + 1 on the periodic line, the in-range ones on the interval
__host__ __device__ inline int64_t line_prior_count(const BurgersLinePriorArgs& a, int64_t i, int64_t R) {
    if (a.periodic) return 2 * R + 1;
    return (i < R ? i : R) + 1 + (a.ns - 1 - i < R ? a.ns - 1 - i : R);
}

// sum of line_prior_count over the columns j < i
__host__ __device__ inline int64_t line_prior_prefix(const BurgersLinePriorArgs& a, int64_t i, int64_t R) {
    if (a.periodic) return (2 * R + 1) * i;
    auto tri = [R](int64_t m) { return m <= R + 1 ? m * (m - 1) / 2 : R * (R + 1) / 2 + (m - R - 1) * R; };     // sum_{j<m} min(j, R)
    return i + tri(i) + tri(a.ns) - tri(a.ns - i);
}

// first entry of slice t's columns, and of column i within them
__host__ __device__ inline int64_t line_prior_slice_start(const BurgersLinePriorArgs& a, int64_t t) {
    const int64_t nd = line_prior_prefix(a, a.ns, 2 * a.order), nb = line_prior_prefix(a, a.ns, a.order);
    return t * nd + ((t > 0 ? t - 1 : 0) + t) * nb;
}

__host__ __device__ inline int64_t line_prior_col_start(const BurgersLinePriorArgs& a, int64_t t, int64_t i) {
    const int64_t beside = (t > 0 ? 1 : 0) + (t < a.nt - 1 ? 1 : 0);
    return line_prior_prefix(a, i, 2 * a.order) + beside * line_prior_prefix(a, i, a.order);
}

inline int64_t burgers_line_prior_nnz(const BurgersLinePriorArgs& a) { return line_prior_slice_start(a, a.nt - 1) + line_prior_col_start(a, a.nt - 1, a.ns); }

__host__ __device__ inline int64_t burgers_line_prior_colptr(const BurgersLinePriorArgs& a, int64_t t, int64_t i) {
    return line_prior_slice_start(a, t) + line_prior_col_start(a, t, i);
}

// (row, column) of stored entry e: the one statement of the pattern, for the host's CSC arrays and the value kernel alike
__host__ __device__ inline void burgers_line_prior_entry(const BurgersLinePriorArgs& a, int64_t e, int64_t* row, int64_t* col) {
    const int64_t ns = a.ns, first = line_prior_slice_start(a, 1);
    int64_t t = 0;
    if (e >= first) {
        const int64_t mid = line_prior_slice_start(a, 2) - first;     // (the size of a slice with both neighbours)
        t = 1 + (e - first) / mid;
        if (t > a.nt - 1) t = a.nt - 1;
    }
    const int64_t r = e - line_prior_slice_start(a, t);
    int64_t lo = 0, hi = ns - 1;        // the last column that starts at or before r
    while (lo < hi) {
        const int64_t m = (lo + hi + 1) / 2;
        if (line_prior_col_start(a, t, m) <= r) lo = m; else hi = m - 1;
    }
    const int64_t i = lo;
    int64_t k = r - line_prior_col_start(a, t, i), blk, R;
    const int64_t before = t > 0 ? line_prior_count(a, i, a.order) : 0, own = line_prior_count(a, i, 2 * a.order);
    if (k < before) { blk = t - 1; R = a.order; }
    else if (k < before + own) { k -= before; blk = t; R = 2 * a.order; }
    else { k -= before + own; blk = t + 1; R = a.order; }
    int64_t rk;                         // the k-th smallest of the rows i - R .. i + R, wrapped or clipped
    if (!a.periodic) rk = (i > R ? i - R : 0) + k;
    else if (i - R < 0) rk = k <= i + R ? k : ns + i - R + (k - (i + R + 1));
    else if (i + R >= ns) { const int64_t nw = i + R - ns + 1; rk = k < nw ? k : i - R + (k - nw); }
    else rk = i - R + k;
    *row = blk * ns + rk;
    *col = t * ns + i;
}

// ------------------------------------------------------------------------------------------------ the line's operators
// Element matrices in the dof order (left, right) / (left, right, middle), by the cell length h: mass h/6 [2 1; 1 2] and
// h/30 [4 -1 2; -1 4 2; 2 2 16], stiffness 1/h [1 -1; -1 1] and 1/(3h) [7 1 -8; 1 7 -8; -8 -8 16], advection 1/2 [-1 1; -1 1] and
// 1/6 [-3 -1 4; 1 3 -4; -4 4 0].  Cell e holds the positions order e .. order e + order; a cell of the periodic line is addressed by
// positions that are not wrapped (the matrices do not depend on e), a cell of the interval exists for 0 <= e < nc.
__host__ __device__ inline int line_prior_local(int order, int64_t u) { return order == 1 ? (int)u : (u == 0 ? 0 : (u == 2 ? 1 : 2)); }

__host__ __device__ inline double line_prior_mass_rowsum(int order, double h, int li) {
    if (order == 1) return h / 6.0 * 2.0 + h / 6.0 * 1.0;
    const double m = h / 30.0;
    return li == 2 ? m * 2.0 + m * 2.0 + m * 16.0 : (li == 0 ? m * 4.0 + m * -1.0 + m * 2.0 : m * -1.0 + m * 4.0 + m * 2.0);
}

__host__ __device__ inline void line_prior_cells(const BurgersLinePriorArgs& a, int64_t i, int64_t* e0, int* count) {
    if (a.order == 1) { *e0 = i - 1; *count = 2; }
    else if (i & 1) { *e0 = (i - 1) / 2; *count = 1; }
    else { *e0 = i / 2 - 1; *count = 2; }
}

// l_i: the cells' row sums of the mass, left cell first
__host__ __device__ inline double line_prior_lumped(const BurgersLinePriorArgs& a, int64_t i) {
    int64_t e0; int count;
    line_prior_cells(a, i, &e0, &count);
    double l = 0.0;
    for (int c = 0; c < count; ++c) {
        const int64_t e = e0 + c;
        if (!a.periodic && (e < 0 || e >= a.nc)) continue;
        l += line_prior_mass_rowsum(a.order, a.h, line_prior_local(a.order, i - a.order * e));
    }
    return l;
}

// S[i][i + d] and Adv[i][i + d], the cells' contributions added left cell first; 0.0 where the two dofs share no cell
__host__ __device__ inline void line_prior_sa(const BurgersLinePriorArgs& a, int64_t i, int64_t d, double* s_out, double* adv_out) {
    const double S1[2][2] = {{1.0, -1.0}, {-1.0, 1.0}}, A1[2][2] = {{-1.0, 1.0}, {-1.0, 1.0}};
    const double S2[3][3] = {{7.0, 1.0, -8.0}, {1.0, 7.0, -8.0}, {-8.0, -8.0, 16.0}}, A2[3][3] = {{-3.0, -1.0, 4.0}, {1.0, 3.0, -4.0}, {-4.0, 4.0, 0.0}};
    int64_t e0; int count;
    line_prior_cells(a, i, &e0, &count);
    double s = 0.0, adv = 0.0;
    for (int c = 0; c < count; ++c) {
        const int64_t e = e0 + c;
        if (!a.periodic && (e < 0 || e >= a.nc)) continue;
        const int64_t ui = i - a.order * e, uj = ui + d;
        if (uj < 0 || uj > a.order) continue;
        const int li = line_prior_local(a.order, ui), lj = line_prior_local(a.order, uj);
        if (a.order == 1) { s += 1.0 / a.h * S1[li][lj]; adv += 0.5 * A1[li][lj]; }
        else { s += 1.0 / (3.0 * a.h) * S2[li][lj]; adv += A2[li][lj] / 6.0; }
    }
    *s_out = s; *adv_out = adv;
}

// the scalars of one problem, written as the host statement writes them
struct BurgersLinePriorCoef {
    double nuc, gamma, kappa2, wnum;    // w_k = wnum / l_k
};

__host__ __device__ inline BurgersLinePriorCoef burgers_line_prior_coef(const BurgersLinePriorArgs& a, double bulk) {
    const double c = 1.0 / a.nu, tau = 0.1 * sqrt(c);
    BurgersLinePriorCoef k;
    k.nuc = a.nu * c; k.gamma = -c * bulk; k.kappa2 = 12.0 * (double)a.nc; k.wnum = 1.0 / (a.dt * tau * tau);
    return k;
}

// G[k][k + d] and K[k][k + d]
__host__ __device__ inline double line_prior_G(const BurgersLinePriorArgs& a, const BurgersLinePriorCoef& q, int64_t k, int64_t d, double lk) {
    double s, adv;
    line_prior_sa(a, k, d, &s, &adv);
    const double g = a.dt * (q.nuc * s + q.gamma * adv);
    return d == 0 ? lk + g : g;
}

__host__ __device__ inline double line_prior_K(const BurgersLinePriorArgs& a, const BurgersLinePriorCoef& q, int64_t k, int64_t d, double lk) {
    double s, adv;
    line_prior_sa(a, k, d, &s, &adv);
    return d == 0 ? q.kappa2 * lk + s : s;
}

// j - k on the line: the signed distance of least absolute value on the periodic line
__host__ __device__ inline int64_t line_prior_dist(const BurgersLinePriorArgs& a, int64_t k, int64_t j) {
    int64_t d = j - k;
    if (a.periodic) { if (2 * d > a.ns) d -= a.ns; else if (2 * d < -a.ns) d += a.ns; }
    return d;
}

__host__ __device__ inline bool line_prior_observed(const BurgersLinePriorArgs& a, int64_t i) {
    if (!a.periodic && (i == 0 || i == a.ns - 1)) return false;
    return !(a.vertices && (i & 1));
}

__host__ __device__ inline int64_t line_prior_observed_count(const BurgersLinePriorArgs& a) {
    if (a.vertices) return a.periodic ? a.ns / 2 : (a.ns + 1) / 2 - 2;
    return a.periodic ? a.ns : a.ns - 2;
}

// Entry (row, col) of Q_ic; `closed`: with the pins and ic_noise (the stored values), without them the Q_prior of the information
// vector.  The entry is evaluated for the pair (smaller index, larger index) of its two dofs -- in a block beside the diagonal
// (earlier slice's dof, later slice's dof) -- so that (row, col) and (col, row) take the same path with the same arguments: the
// values are bitwise symmetric.  The shared rows k = lo - order .. lo + order go in ascending index: on the periodic line the ones
// wrapped from beyond ns-1 first, those wrapped from below 0 last.
__host__ __device__ inline double burgers_line_prior_value(const BurgersLinePriorArgs& a, const BurgersLinePriorCoef& q, int64_t row, int64_t col,
                                                           bool closed) {
    const int64_t ns = a.ns, tr = row / ns, ia = row % ns, tc = col / ns, ib = col % ns, R = a.order;
    if (tr != tc) {                     // -(G' W diag(l))[later][earlier] = -(G[b][a] w_b) l_b, b the earlier slice's dof
        const int64_t b = tr > tc ? ib : ia, later = tr > tc ? ia : ib;
        const double lb = line_prior_lumped(a, b);
        return -((line_prior_G(a, q, b, line_prior_dist(a, b, later), lb) * (q.wnum / lb)) * lb);
    }
    const int64_t lo = ia < ib ? ia : ib, hi = ia < ib ? ib : ia;
    double v = 0.0;
    for (int pass = 0; pass < 3; ++pass)
        for (int64_t o = -R; o <= R; ++o) {
            int64_t k = lo + o;
            const int where = k >= ns ? 0 : (k >= 0 ? 1 : 2);
            if (where != pass) continue;
            if (where != 1) {
                if (!a.periodic) continue;
                k += where == 0 ? -ns : ns;
            }
            const int64_t dh = line_prior_dist(a, k, hi);
            if (dh < -R || dh > R) continue;
            const double lk = line_prior_lumped(a, k);
            if (tr == 0) v += (line_prior_K(a, q, k, -o, lk) * (1.0 / lk)) * line_prior_K(a, q, k, dh, lk);
            else v += (line_prior_G(a, q, k, -o, lk) * (q.wnum / lk)) * line_prior_G(a, q, k, dh, lk);
        }
    if (ia == ib) {
        if (tr < a.nt - 1) { const double l = line_prior_lumped(a, ia); v += (l * (q.wnum / l)) * l; }
        if (closed) {
            if (!a.periodic && (ia == 0 || ia == ns - 1)) v += a.pin;
            if (tr == 0 && line_prior_observed(a, ia)) v += a.ic_noise;
        }
    }
    return v;
}

// ------------------------------------------------------------------------------------------------ kernels
// bulk[p] = mean of ic[p] over the observed dofs: burgers_bulk_batch's fixed shape -- thread t adds its observed dofs among
// t, t + 256, ... in order, then the fixed tree -- so that with every dof observed the bits are that kernel's.
__global__ __launch_bounds__(256) void burgers_line_bulk_batch(BurgersLinePriorArgs a, const double* __restrict__ ic, double* __restrict__ bulk) {
    __shared__ double red[256];
    const int64_t p = blockIdx.y;
    ic += p * a.ns;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < a.ns; i += 256)
        if (line_prior_observed(a, i)) acc += ic[i];
    const double sum = block_sum_256(acc, red);
    if (threadIdx.x == 0) bulk[p] = sum / (double)line_prior_observed_count(a);
}

// q[p][e]: one thread per stored entry
__global__ __launch_bounds__(256) void burgers_line_prior_values_batch(BurgersLinePriorArgs a, const double* __restrict__ bulk, int64_t nnz,
                                                                       double* __restrict__ q) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    const int64_t p = blockIdx.y;
    const BurgersLinePriorCoef k = burgers_line_prior_coef(a, bulk[p]);
    int64_t row, col;
    burgers_line_prior_entry(a, e, &row, &col);
    q[p * nnz + e] = burgers_line_prior_value(a, k, row, col, true);
}

// (row r of Q_prior(without the pins)) 1: the row's entries added slice t-1, t, t+1 in turn, columns ascending (the wrapped ones as
// in burgers_line_prior_value)
__host__ __device__ inline double burgers_line_prior_row_sum(const BurgersLinePriorArgs& a, const BurgersLinePriorCoef& k, int64_t r) {
    const int64_t ns = a.ns, t = r / ns, i = r % ns;
    double s = 0.0;
    for (int64_t tc = t - 1; tc <= t + 1; ++tc) {
        if (tc < 0 || tc >= a.nt) continue;
        const int64_t R = tc == t ? 2 * a.order : a.order;
        for (int pass = 0; pass < 3; ++pass)
            for (int64_t o = -R; o <= R; ++o) {
                int64_t c = i + o;
                const int where = c >= ns ? 0 : (c >= 0 ? 1 : 2);
                if (where != pass) continue;
                if (where != 1) {
                    if (!a.periodic) continue;
                    c += where == 0 ? -ns : ns;
                }
                s += burgers_line_prior_value(a, k, r, tc * ns + c, false);
            }
    }
    return s;
}

// qx[p][r] = ((row r of Q_prior) 1) bulk_p + ic_noise [ic_p at the observed dofs; 0]_r: one thread per row
__global__ __launch_bounds__(256) void burgers_line_prior_rhs_batch(BurgersLinePriorArgs a, const double* __restrict__ bulk,
                                                                    const double* __restrict__ ic, double* __restrict__ qx) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, ns = a.ns, n = ns * a.nt;
    if (r >= n) return;
    const int64_t p = blockIdx.y;
    const double b = bulk[p];
    double v = burgers_line_prior_row_sum(a, burgers_line_prior_coef(a, b), r) * b;
    if (r < ns && line_prior_observed(a, r)) v += a.ic_noise * ic[p * ns + r];
    qx[p * n + r] = v;
}

}  // namespace gmrf
