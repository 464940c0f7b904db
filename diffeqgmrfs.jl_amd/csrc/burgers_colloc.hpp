// Residual and tangent of the implicit-Euler Burgers system evaluated at collocation points on the periodic quadratic line:
// f_and_J of scripts/burgers/solve_burgers_gmrf-collocation.jl:186-192 with J_static (:183), the operators A_coll, du/dx and
// d2u/dx2 of :167-169 restated per point by the shape functions of the cell that holds it.
//
// Mesh: the periodic quadratic line of burgers_line.hpp -- nc cells of length h, ns = 2 nc dofs numbered by position, cell e with
// the dofs (left, right, middle) = (2e, (2e+2) mod ns, 2e+1).  A point x_c lies in the cell e_c = min(floor(x_c / h), nc - 1) at
// xi = 2 (x_c - e_c h) / h - 1; its shape values a = (xi(xi-1)/2, xi(xi+1)/2, 1 - xi^2), first derivatives
// d = (xi - 1/2, xi + 1/2, -2 xi) 2/h and second derivatives s = (1, 1, -2) 4/h^2 are computed ONCE, on the host in double
// precision (gmrf_burgers_colloc_create), and uploaded: the pattern and the kernel read the same cell, so they cannot disagree
// on a floor.  The table is stored by local dof, [3][npts], so that consecutive threads read consecutive words.
//
// Row r = (t-1) npts + c of the step t-1 -> t (t = 1 .. nt-1, 0-based), with u = sum a_k w_t[k], u_x = sum d_k w_t[k],
// u_xx = sum s_k w_t[k], u- = sum a_k w_{t-1}[k], every sum in the LOCAL order (left, right, middle):
//   f_r          = u - u- + dt u u_x - dt nu u_xx
//   J[r, t-1, k] = -a_k
//   J[r, t,   k] = a_k + dt (u_x a_k + u d_k) - dt nu s_k
// Six stored entries per row: the cell's three dofs of slice t-1 in ascending column order, then of slice t.  Ascending is
// (left, middle, right) = (2e, 2e+1, 2e+2) except in the wrap cell e = nc-1, whose right dof is 0: (right, left, middle).  An
// entry that is exactly 0.0 (a point on a vertex) is stored.
//
// Structure of the other tangent kernels: one thread per row, gather, no atomics, fixed summation order; blockIdx.y is the
// problem, and the one-problem call is the batch kernel with one problem.  Several points may share a cell: rows are independent.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gmrf {

struct BurgersCollocArgs {
    int ns, nt, npts;
    double dt, nu;
    double s[3];                    // second derivatives of the shape functions, local order: (1, 1, -2) 4/h^2
    const int32_t* cell;            // [npts]    the cell of every point
    const double* a;                // [3][npts] shape values, by local dof
    const double* d;                // [3][npts] first derivatives
    const double* w;                // [nt * ns]
    double* vals;                   // [6 * rows]
    double* f;                      // [rows], rows = (nt - 1) * npts
};

__device__ __forceinline__ void burgers_colloc_row(const BurgersCollocArgs& p, const int64_t gid) {
    const int64_t rows = (int64_t)(p.nt - 1) * p.npts;
    if (gid >= rows) return;
    const int t = (int)(gid / p.npts) + 1, c = (int)(gid % p.npts);
    const int e = p.cell[c];
    const bool wrap = 2 * e + 2 == p.ns;
    const int cl = 2 * e, cr = wrap ? 0 : 2 * e + 2, cm = 2 * e + 1;
    const double a0 = p.a[c], a1 = p.a[p.npts + c], a2 = p.a[2 * (int64_t)p.npts + c];
    const double d0 = p.d[c], d1 = p.d[p.npts + c], d2 = p.d[2 * (int64_t)p.npts + c];
    const double* wt = p.w + (int64_t)t * p.ns;
    const double* wp = wt - p.ns;
    const double w0 = wt[cl], w1 = wt[cr], w2 = wt[cm];
    const double u = a0 * w0 + a1 * w1 + a2 * w2;
    const double ux = d0 * w0 + d1 * w1 + d2 * w2;
    const double uxx = p.s[0] * w0 + p.s[1] * w1 + p.s[2] * w2;
    const double um = a0 * wp[cl] + a1 * wp[cr] + a2 * wp[cm];
    const double cd = p.dt * p.nu;
    p.f[gid] = u - um + p.dt * u * ux - cd * uxx;
    const double j0 = a0 + p.dt * (ux * a0 + u * d0) - cd * p.s[0];
    const double j1 = a1 + p.dt * (ux * a1 + u * d1) - cd * p.s[1];
    const double j2 = a2 + p.dt * (ux * a2 + u * d2) - cd * p.s[2];
    // the places of (left, right, middle) in the ascending order of the row's three columns
    const int pl = wrap ? 1 : 0, pr = wrap ? 0 : 2, pm = wrap ? 2 : 1;
    double* v = p.vals + gid * 6;
    v[pl] = -a0; v[pr] = -a1; v[pm] = -a2;
    v[3 + pl] = j0; v[3 + pr] = j1; v[3 + pm] = j2;
}

// w[B][nt ns] -> vals[B][6 rows], f[B][rows], problem-major; blockIdx.y is the problem.  One problem is a batch of one.
__global__ __launch_bounds__(256) void burgers_colloc_rows(BurgersCollocArgs p) {
    const int64_t b = blockIdx.y, rows = (int64_t)(p.nt - 1) * p.npts;
    p.w += b * ((int64_t)p.nt * p.ns); p.vals += b * 6 * rows; p.f += b * rows;
    burgers_colloc_row(p, (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
}

}  // namespace gmrf
