// Residual and tangent of the Burgers space-time system on a line, generalised over three independent choices:
//   order   1 (P1) or 2 (quadratic line), the elements of fem_assemble.hpp (burgers_p1_cell / burgers_p2_cell: the reference's
//           quadrature loop, src/problems/burgers.jl:22-51, is theirs and is reused here);
//   scheme  implicit Euler (f_and_J, scripts/burgers/solve_burgers_gmrf-fem.jl:118-149) or Crank-Nicolson (J_static_CN,
//           nonlinear_primal_tangent_CN, f_and_J_CN: _research/burgers_chen24.jl:121-132, :195-226);
//   bc      the periodic line (wrap-around columns) or an interval with homogeneous Dirichlet ends (_research/burgers_chen24.jl:101-108).
// Implicit Euler on the periodic line of length 1 is served by burgers_p1_rows_batch / burgers_p2_rows_batch of fem_assemble.hpp,
// which keep their bits and know that cell length only; the kernels here serve everything else.
//
// Row block of the step t-1 -> t (t = 1 .. nt-1, 0-based), with M, G the consistent mass and stiffness, A(w), v(w) the assembled
// advection tangent and residual of one slice:
//   euler:  J[:, t-1] = -M                              J[:, t] = M + (dt nu) G + dt A(w_t)
//           f = (static part of the row) . w + dt v(w_t)
//   cn:     J[:, t-1] = -M + (dt nu 0.5) G + (dt 0.5) A(w_{t-1})     J[:, t] = M + (dt nu 0.5) G + (dt 0.5) A(w_t)
//           f = (static part of the row) . w + (dt 0.5) (v(w_{t-1}) + v(w_t))
// The static part is the row without its A terms; its product with w is summed in ascending column order, slice t-1 first.
//
// Dirichlet interval: nc cells, ns = order nc + 1 dofs numbered by position; dofs 0 and ns-1 are prescribed and treated as the
// reference treats them (src/problems/burgers.jl:53-57, :87-92: after apply! and the diagonal reset their rows AND columns of M, G
// and A are zero and v vanishes there).  They stay in the system as rows and columns with stored 0.0 and f = 0.0, so
// m = (nt-1) ns stays uniform; the cells are evaluated with the w the caller passes, prescribed dofs included.  A row holds
// its in-range columns only; every interior row has its whole window in range, the two end rows are clipped -- the row pointer
// comes from the host (gmrf_burgers_p1_pattern's) instead of a closed form.
//
// Structure of the kernels of fem_assemble.hpp: one thread per row (t, i), gather, no atomics, fixed summation order; blockIdx.y
// is the problem, and the one-problem call is the batch kernel with one problem.  The row's window of columns i-R .. i+R (R = order;
// a quadratic midpoint row uses the entries 1 .. 3 of its 5) is held in registers under compile-time indices: the ascending
// order after the periodic wrap-around is a rotation, applied to the store addresses and to the order of the f sum by
// predicates, not by indexing a local array.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fem_assemble.hpp"

namespace gmrf {

struct BurgersLineArgs {
    int ns, nt;
    double dt, nu, h;               // h: cell length
    const int64_t* rowptr;          // dirichlet: 0-based CSR row pointer of J; periodic: unused (closed form)
    const double* w;                // [nt * ns]
    double* vals;                   // [nnz]
    double* f;                      // [(nt - 1) * ns]
};

// one slice's assembled row in the window: mass, stiffness, advection tangent, the slice's w at the window's columns, and v_i
template <int ORDER> struct BurgersLineWindow {
    double m[2 * ORDER + 1], d[2 * ORDER + 1], g[2 * ORDER + 1], w[2 * ORDER + 1], v;
};

template <int ORDER>
__device__ __forceinline__ void burgers_line_window(double h, const double* __restrict__ ws, const int (&col)[2 * ORDER + 1], bool mid,
                                                    BurgersLineWindow<ORDER>& r) {
    if constexpr (ORDER == 1) {
        r.w[0] = ws[col[0]]; r.w[1] = ws[col[1]]; r.w[2] = ws[col[2]];
        double GeL[2][2], veL[2], MeL[2][2], DeL[2][2], GeR[2][2], veR[2], MeR[2][2], DeR[2][2];
        burgers_p1_cell(h, r.w[0], r.w[1], GeL, veL, MeL, DeL);       // cell (i-1, i): this node is local 1
        burgers_p1_cell(h, r.w[1], r.w[2], GeR, veR, MeR, DeR);       // cell (i, i+1): this node is local 0
        r.m[0] = MeL[1][0]; r.m[1] = MeL[1][1] + MeR[0][0]; r.m[2] = MeR[0][1];
        r.d[0] = DeL[1][0]; r.d[1] = DeL[1][1] + DeR[0][0]; r.d[2] = DeR[0][1];
        r.g[0] = GeL[1][0]; r.g[1] = GeL[1][1] + GeR[0][0]; r.g[2] = GeR[0][1];
        r.v = veL[1] + veR[0];
    } else {
        double Ge[3][3], ve[3], Me[3][3], De[3][3];
        r.w[1] = ws[col[1]]; r.w[2] = ws[col[2]]; r.w[3] = ws[col[3]];
        if (mid) {                                      // midpoint of its own cell: local dof 2; columns left, middle, right = local 0, 2, 1
            r.w[0] = 0.0; r.w[4] = 0.0;
            const double w3[3] = {r.w[1], r.w[3], r.w[2]};
            burgers_p2_cell(h, w3, Ge, ve, Me, De);
            r.m[0] = 0.0; r.m[1] = Me[2][0]; r.m[2] = Me[2][2]; r.m[3] = Me[2][1]; r.m[4] = 0.0;
            r.d[0] = 0.0; r.d[1] = De[2][0]; r.d[2] = De[2][2]; r.d[3] = De[2][1]; r.d[4] = 0.0;
            r.g[0] = 0.0; r.g[1] = Ge[2][0]; r.g[2] = Ge[2][2]; r.g[3] = Ge[2][1]; r.g[4] = 0.0;
            r.v = ve[2];
        } else {                                        // vertex: right end (local 1) of the left cell, left end (local 0) of the right cell
            r.w[0] = ws[col[0]]; r.w[4] = ws[col[4]];
            const double wl[3] = {r.w[0], r.w[2], r.w[1]};
            const double wr[3] = {r.w[2], r.w[4], r.w[3]};
            double GeR[3][3], veR[3], MeR[3][3], DeR[3][3];
            burgers_p2_cell(h, wl, Ge, ve, Me, De);
            burgers_p2_cell(h, wr, GeR, veR, MeR, DeR);
            r.m[0] = Me[1][0]; r.m[1] = Me[1][2]; r.m[2] = Me[1][1] + MeR[0][0]; r.m[3] = MeR[0][2]; r.m[4] = MeR[0][1];
            r.d[0] = De[1][0]; r.d[1] = De[1][2]; r.d[2] = De[1][1] + DeR[0][0]; r.d[3] = DeR[0][2]; r.d[4] = DeR[0][1];
            r.g[0] = Ge[1][0]; r.g[1] = Ge[1][2]; r.g[2] = Ge[1][1] + GeR[0][0]; r.g[3] = GeR[0][2]; r.g[4] = GeR[0][1];
            r.v = ve[1] + veR[0];
        }
    }
}

template <int ORDER, bool CN, bool DIR>
__device__ __forceinline__ void burgers_line_row(const BurgersLineArgs& a, const int64_t gid) {
    constexpr int W = 2 * ORDER + 1;
    const int64_t rows = (int64_t)(a.nt - 1) * a.ns;
    if (gid >= rows) return;
    const int ns = a.ns;
    const int t = (int)(gid / ns) + 1, i = (int)(gid % ns);       // slice t (0-based), rows belong to slices 1 .. nt-1
    if (DIR && (i == 0 || i == ns - 1)) {                          // a prescribed dof: its clipped row holds zeros
        for (int64_t e = a.rowptr[gid]; e < a.rowptr[gid + 1]; ++e) a.vals[e] = 0.0;
        a.f[gid] = 0.0;
        return;
    }
    const bool mid = ORDER == 2 && (i & 1);
    const int k0 = mid ? 1 : 0, cnt = mid ? 3 : W;                 // the row's entries of the window: k0 .. k0 + cnt - 1
    // columns of the window; periodic: wrapped, and the ascending order is the window rotated by `first` entries.  Dirichlet: an
    // interior row's entries are in range; the two unused entries of a midpoint row's window are clamped, never out of range
    int col[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const int c = i - ORDER + k;
        col[k] = DIR ? min(max(c, 0), ns - 1) : (c < 0 ? c + ns : (c >= ns ? c - ns : c));
    }
    int first = 0;
    if (!DIR) {
        const int half = cnt / 2, nneg = half - i, nover = i + half - (ns - 1);
        first = nneg > 0 ? nneg : (nover > 0 ? cnt - nover : 0);
    }
    const double* wt = a.w + (int64_t)t * ns;
    const double* wp = a.w + (int64_t)(t - 1) * ns;
    BurgersLineWindow<ORDER> cur, prev;
    burgers_line_window<ORDER>(a.h, wt, col, mid, cur);
    if (CN) burgers_line_window<ORDER>(a.h, wp, col, mid, prev);
    else {
#pragma unroll
        for (int k = 0; k < W; ++k) prev.w[k] = (k >= k0 && k < k0 + cnt) ? wp[col[k]] : 0.0;
    }
    const double cd = CN ? a.dt * a.nu * 0.5 : a.dt * a.nu, cg = CN ? a.dt * 0.5 : a.dt;
    int64_t base;
    if (DIR) base = a.rowptr[gid];
    else base = ORDER == 2 ? burgers_p2_row_offset(ns, t - 1, i) : gid * 6;
    double* v = a.vals + base;
    double tp[W], tc[W];                                           // the terms of (static row) . w
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const int c = k - k0;
        if (c < 0 || c >= cnt) { tp[k] = 0.0; tc[k] = 0.0; continue; }
        double sp = CN ? -cur.m[k] + cd * cur.d[k] : -cur.m[k];    // M and G do not depend on the slice
        double st = cur.m[k] + cd * cur.d[k];
        double jp = CN ? sp + cg * prev.g[k] : sp;
        double jc = st + cg * cur.g[k];
        if (DIR && (col[k] == 0 || col[k] == ns - 1)) { sp = 0.0; st = 0.0; jp = 0.0; jc = 0.0; }      // a prescribed column
        const int pos = c - first + (c < first ? cnt : 0);
        v[pos] = jp;
        v[cnt + pos] = jc;
        tp[k] = sp * prev.w[k];
        tc[k] = st * cur.w[k];
    }
    // ascending column order, slice t-1 first: the rotated window starts at entry `first`
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < W; ++k) if (k - k0 >= first && k - k0 < cnt) acc += tp[k];
#pragma unroll
    for (int k = 0; k < W; ++k) if (k - k0 >= 0 && k - k0 < first) acc += tp[k];
#pragma unroll
    for (int k = 0; k < W; ++k) if (k - k0 >= first && k - k0 < cnt) acc += tc[k];
#pragma unroll
    for (int k = 0; k < W; ++k) if (k - k0 >= 0 && k - k0 < first) acc += tc[k];
    a.f[gid] = CN ? acc + cg * (prev.v + cur.v) : acc + cg * cur.v;
}

// w[B][nt ns] -> vals[B][nnz], f[B][rows], problem-major; blockIdx.y is the problem.  One problem is a batch of one.
template <int ORDER, bool CN, bool DIR>
__global__ __launch_bounds__(256) void burgers_line_rows(BurgersLineArgs a, int64_t nnz) {
    const int64_t p = blockIdx.y, rows = (int64_t)(a.nt - 1) * a.ns;
    a.w += p * ((int64_t)a.nt * a.ns); a.vals += p * nnz; a.f += p * rows;
    burgers_line_row<ORDER, CN, DIR>(a, (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
}

}  // namespace gmrf
