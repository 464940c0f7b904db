// FEM block assembly on the device, fourth piece: tangent, residual and load of the nonlinear elliptic benchmark
//     -Lap u + u^3 = f_src        (/root/reference/_research/elliptic_chen24.jl)
// as the reference's Gauss-Newton loop evaluates them per iteration (`f_and_J`, :280-285):
//     J(w) = J_static + J_cube(w),   J_static[i][j] = int grad(phi_i) . grad(phi_j)            (assemble_J_diff_and_f, :179-228)
//                                    J_cube[i][j]   = int 3 phi_i u_h^2 phi_j                  (assemble_J_cube, :231-278)
//     f(w) = J_static w + int phi_i u_h^3                                                     (:282 without the load)
//     b[i] = int phi_i f_src                                                                  (the `fe` of :222)
// The load is not part of f: it reaches the Gauss-Newton driver as the observations y, obs_diff = y - f(x), which is the
// reference's `J_static w + f_cube - f_static` against zero observations.
//
// Mesh and conventions are those of swe_assemble.hpp: nx x ny nodes on the unit square, x fastest, every quad cut by the
// diagonal n00 - n11 into the P1 triangles (n00, n10, n11) [cell qy (nx-1) + qx] and (n00, n11, n01) [cell (nx-1)(ny-1) +
// qy (nx-1) + qx]; the symmetric 3-point rule (QuadratureRule{RefTriangle}(element_order + 1) of :122 for P1): dOmega =
// |T| / 3, point q has the barycentric weight 2/3 on cell vertex 2 - q and 1/6 on the other two.  The source enters through
// its values at the quadrature points, src_q[cell][q].  Prescribed dofs are the nodes on the four sides: their ROWS are
// skipped and stay zero (`continue`, :210-212 and :262-264), columns are kept, no apply! is done.
//
// Gather instead of scatter, as in the Darcy, Burgers and shallow-water kernels: a thread owns one node row, walks the
// node's (at most six) cells in ascending cell number, forms per cell the element row in quadrature order and adds it to
// the row's stencil slots: fixed summation order, no atomics.  The 7-point stencil is the row's CSR entry list in ascending
// column order -- the pattern of darcy_p1_row, explicit zeros included.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fem_assemble.hpp"

namespace gmrf {

struct EllipticP1Args {
    int nx, ny;
    const int64_t* rowptr;          // CSR of the 7-point stencil
    const double* w;                // [n] linearisation point
    double* vals;                   // [nnz]
    double* f;                      // [n]
};

struct EllipticLoadArgs {
    int nx, ny;
    const double* src;              // [cells][3]
    double* b;                      // [n]
};

// Floating-point contraction is switched off in every function below (as in lin_coord): a row then rounds as the host oracle
// does, whatever the compiler would otherwise fuse in the kernel it is inlined into.

// signed 2 |T| of one cell as the determinant of the cell Jacobian (as in swe_p1_rows), with the coefficients of the P1 gradients
__device__ __forceinline__ double elliptic_cell_area2(int nx, int ny, const int (&nxs)[3], const int (&nys)[3], double (&b)[3], double (&c)[3]) {
#pragma clang fp contract(off)
    double x[3], y[3];
#pragma unroll
    for (int v = 0; v < 3; ++v) { x[v] = lin_coord(nxs[v], nx); y[v] = lin_coord(nys[v], ny); }
    b[0] = y[1] - y[2]; b[1] = y[2] - y[0]; b[2] = y[0] - y[1];
    c[0] = x[2] - x[1]; c[1] = x[0] - x[2]; c[2] = x[1] - x[0];
    return c[2] * b[1] - c[1] * b[2];
}

// dOmega of a quadrature point of one cell: |T| / 3
__device__ __forceinline__ double elliptic_cell_dO(int nx, int ny, const int (&nxs)[3], const int (&nys)[3]) {
#pragma clang fp contract(off)
    double b[3], c[3];
    return 0.5 * fabs(elliptic_cell_area2(nx, ny, nxs, nys, b, c)) / 3.0;
}

// geometry of one cell: gradients of the three shape functions and dOmega of a quadrature point
__device__ __forceinline__ void elliptic_cell_geometry(int nx, int ny, const int (&nxs)[3], const int (&nys)[3], double (&gx)[3],
                                                       double (&gy)[3], double& dO) {
#pragma clang fp contract(off)
    double b[3], c[3];
    const double area2 = elliptic_cell_area2(nx, ny, nxs, nys, b, c);
    dO = 0.5 * fabs(area2) / 3.0;
#pragma unroll
    for (int v = 0; v < 3; ++v) { gx[v] = b[v] / area2; gy[v] = c[v] / area2; }
}

__device__ __forceinline__ void elliptic_p1_row(const EllipticP1Args& a, const int64_t i) {
#pragma clang fp contract(off)
    const int64_t n = (int64_t)a.nx * a.ny;
    if (i >= n) return;
    const int ix = (int)(i % a.nx), iy = (int)(i / a.nx);
    const bool has[7] = {ix > 0 && iy > 0, iy > 0, ix > 0, true, ix < a.nx - 1, iy < a.ny - 1, ix < a.nx - 1 && iy < a.ny - 1};
    int64_t p = a.rowptr[i];
    if (ix == 0 || iy == 0 || ix == a.nx - 1 || iy == a.ny - 1) {          // prescribed: the row stays zero
#pragma unroll
        for (int s = 0; s < 7; ++s)
            if (has[s]) a.vals[p++] = 0.0;
        a.f[i] = 0.0;
        return;
    }
    // an interior node: all six cells and all seven stencil neighbours exist
    double sslot[7] = {0, 0, 0, 0, 0, 0, 0}, cslot[7] = {0, 0, 0, 0, 0, 0, 0};
    double vi = 0.0;
    const int cq[6][4] = {{-1, -1, 0, 2}, {-1, 0, 0, 1}, {0, 0, 0, 0}, {-1, -1, 1, 1}, {0, -1, 1, 2}, {0, 0, 1, 0}};
#pragma unroll
    for (int e = 0; e < 6; ++e) {
        const int qx = ix + cq[e][0], qy = iy + cq[e][1];
        const bool upper = cq[e][2] != 0;
        const int li = cq[e][3];
        const int nxs[3] = {qx, qx + 1, upper ? qx : qx + 1};
        const int nys[3] = {qy, upper ? qy + 1 : qy, qy + 1};
        double gx[3], gy[3], dO;
        elliptic_cell_geometry(a.nx, a.ny, nxs, nys, gx, gy, dO);
        double wc[3];                                           // cur_weights[celldofs(cell)] (:253)
#pragma unroll
        for (int v = 0; v < 3; ++v) wc[v] = a.w[(int64_t)nys[v] * a.nx + nxs[v]];
        double se[3] = {0, 0, 0}, ce[3] = {0, 0, 0}, ve = 0.0;
#pragma unroll
        for (int qp = 0; qp < 3; ++qp) {
            double cur_u = 0.0;                                 // function_value (:259)
#pragma unroll
            for (int v = 0; v < 3; ++v) cur_u += ((v == 2 - qp) ? (2.0 / 3.0) : (1.0 / 6.0)) * wc[v];
            const double cur_u_sq = cur_u * cur_u;
            const double phi_i = (li == 2 - qp) ? (2.0 / 3.0) : (1.0 / 6.0);
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                const double phi_j = (v == 2 - qp) ? (2.0 / 3.0) : (1.0 / 6.0);
                se[v] += (gx[v] * gx[li] + gy[v] * gy[li]) * dO;             // :220
                ce[v] += 3.0 * phi_i * cur_u_sq * phi_j * dO;                // :270
            }
            ve += phi_i * (cur_u_sq * cur_u) * dO;                           // :272
        }
#pragma unroll
        for (int v = 0; v < 3; ++v) {                           // assemble! (:225, :275)
            const int s = stencil_slot(nxs[v] - ix, nys[v] - iy);
            sslot[s] += se[v];
            cslot[s] += ce[v];
        }
        vi += ve;
    }
    // J = J_static + J_cube; f = J_static w + f_cube, the product summing the row in ascending column order
    const int dxs[7] = {-1, 0, -1, 0, 1, 0, 1}, dys[7] = {-1, -1, 0, 0, 0, 1, 1};
    double acc = 0.0;
#pragma unroll
    for (int s = 0; s < 7; ++s) {
        a.vals[p++] = sslot[s] + cslot[s];
        acc += sslot[s] * a.w[(int64_t)(iy + dys[s]) * a.nx + (ix + dxs[s])];
    }
    a.f[i] = acc + vi;
}

// A batch of linearisation points on one mesh, problem-major: w[B][n] -> vals[B][nnz], f[B][n]; blockIdx.y is the problem
// (a one-problem call is a batch of 1).  A row's arithmetic does not depend on the problem's place in the batch.
__global__ __launch_bounds__(256) void elliptic_p1_rows_batch(EllipticP1Args a, int64_t nnz) {
    const int64_t p = blockIdx.y, n = (int64_t)a.nx * a.ny;
    a.w += p * n; a.vals += p * nnz; a.f += p * n;
    elliptic_p1_row(a, (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
}

// b[i] = int phi_i f_src over the node's cells (:222); prescribed rows stay zero
__device__ __forceinline__ void elliptic_p1_load_row(const EllipticLoadArgs& a, const int64_t i) {
#pragma clang fp contract(off)
    const int64_t n = (int64_t)a.nx * a.ny;
    if (i >= n) return;
    const int ix = (int)(i % a.nx), iy = (int)(i / a.nx);
    if (ix == 0 || iy == 0 || ix == a.nx - 1 || iy == a.ny - 1) { a.b[i] = 0.0; return; }
    const int cq[6][4] = {{-1, -1, 0, 2}, {-1, 0, 0, 1}, {0, 0, 0, 0}, {-1, -1, 1, 1}, {0, -1, 1, 2}, {0, 0, 1, 0}};
    const int64_t nlow = (int64_t)(a.nx - 1) * (a.ny - 1);
    double bi = 0.0;
#pragma unroll
    for (int e = 0; e < 6; ++e) {
        const int qx = ix + cq[e][0], qy = iy + cq[e][1];
        const bool upper = cq[e][2] != 0;
        const int li = cq[e][3];
        const int nxs[3] = {qx, qx + 1, upper ? qx : qx + 1};
        const int nys[3] = {qy, upper ? qy + 1 : qy, qy + 1};
        const double dO = elliptic_cell_dO(a.nx, a.ny, nxs, nys);
        const int64_t cell = (upper ? nlow : 0) + (int64_t)qy * (a.nx - 1) + qx;
        double fe = 0.0;
#pragma unroll
        for (int qp = 0; qp < 3; ++qp) fe += ((li == 2 - qp) ? (2.0 / 3.0) : (1.0 / 6.0)) * a.src[cell * 3 + qp] * dO;
        bi += fe;
    }
    a.b[i] = bi;
}

// src[B][cells][3] -> b[B][n]; blockIdx.y is the problem (B = 1: the one-problem call)
__global__ __launch_bounds__(256) void elliptic_p1_load_batch(EllipticLoadArgs a) {
    const int64_t p = blockIdx.y, n = (int64_t)a.nx * a.ny;
    a.src += p * (6 * (int64_t)(a.nx - 1) * (a.ny - 1)); a.b += p * n;
    elliptic_p1_load_row(a, (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
}

}  // namespace gmrf
