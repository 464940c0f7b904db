// FEM block assembly on the device, quadratic triangles for the nonlinear elliptic benchmark: the tangent, residual and load of
// elliptic_assemble.hpp (`f_and_J`, _research/elliptic_chen24.jl:280-285 of the reference, with assemble_J_cube :231-278 and
// assemble_J_diff_and_f :179-228) with the reference's default element -- `element_order = 2` of gmrf_fem_solve (:118-122):
// `Lagrange{RefTriangle,2}` and `QuadratureRule{RefTriangle}(3)`.
//
// Mesh, lattice, local node order and the 4-point rule are those of fem_assemble_p2.hpp, whose p2_tri_shape_grad, p2_cell_nodes,
// p2_class_cell and p2_tri_qpoint are used as they are.  Per cell and quadrature point, in the rule's order:
//     cur_u     = sum_v N_v w[celldofs]                  (:259)
//     Je[i][j] += 3 N_i cur_u^2 N_j dOmega               (:270)
//     ve[i]    += N_i cur_u^3 dOmega                     (:272)
//     Se[i][j] += (grad N_j . grad N_i) dOmega           (:220)
//     fe[i]    += N_i src_q dOmega                       (:222)
// Prescribed dofs are the lattice points on the four sides: their ROWS are skipped and stay zero, columns are kept, no apply! is
// done (:210-212, :262-264).
//
// Gather instead of scatter: a thread owns one lattice row, walks the row's cells (6 for a vertex, 2 for an edge or diagonal
// midpoint) in ascending cell number and adds the element row to a 5 x 5 window of lattice offsets; static and cubic parts are
// kept apart (as sslot / cslot of the P1 row) because f needs the static part alone.  The row function is specialised on the dof
// class (the parities of I and J) and fully unrolled: every window index is a compile-time constant, so the windows live in
// registers and only the touched entries exist.  An interior lattice point has all of its cells, so the window's touched
// entries -- written in ascending column order, the CSR order of the Darcy P2 pattern -- depend on the class alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fem_assemble_p2.hpp"

namespace gmrf {

struct EllipticP2Args {
    int nx, ny;                     // vertices per direction
    const int64_t* rowptr;          // CSR of the lattice coupling pattern (darcy_p2_pattern)
    const double* w;                // [n] linearisation point, n = (2 nx - 1)(2 ny - 1)
    double* vals;                   // [nnz]
    double* f;                      // [n]
};

struct EllipticP2LoadArgs {
    int nx, ny;
    const double* src;              // [cells][4]
    double* b;                      // [n]
};

// Floating-point contraction is switched off in every function below, as in elliptic_assemble.hpp: a row then rounds as the host
// oracle does, whatever the compiler would otherwise fuse in the kernel it is inlined into.  (The shape functions of
// fem_assemble_p2.hpp are evaluated at literal quadrature points and fold to constants.)

// the affine geometry of the cell whose nodes have the lattice coordinates (I0 + rI, J0 + rJ): det J and J^-1 with
// J = [x_1 - x_3, x_2 - x_3] as in darcy_p2_row
struct P2CellGeom { double det, i00, i01, i10, i11; };      // J^-1 = [[i00, i01], [i10, i11]]
__device__ __forceinline__ P2CellGeom elliptic_p2_cell_geom(int nx, int ny, int I0, int J0, const int (&rI)[6], const int (&rJ)[6]) {
#pragma clang fp contract(off)
    const double x1 = lin_coord((I0 + rI[0]) / 2, nx), x2 = lin_coord((I0 + rI[1]) / 2, nx), x3 = lin_coord((I0 + rI[2]) / 2, nx);
    const double y1 = lin_coord((J0 + rJ[0]) / 2, ny), y2 = lin_coord((J0 + rJ[1]) / 2, ny), y3 = lin_coord((J0 + rJ[2]) / 2, ny);
    const double ja = x1 - x3, jb = x2 - x3, jc = y1 - y3, jd = y2 - y3;
    P2CellGeom g;
    g.det = ja * jd - jb * jc;
    g.i00 = jd / g.det; g.i01 = -jb / g.det; g.i10 = -jc / g.det; g.i11 = ja / g.det;
    return g;
}

// One interior row of class (PI, PJ) = (I & 1, J & 1).
template <int PI, int PJ>
__device__ __forceinline__ void elliptic_p2_row_class(const EllipticP2Args& a, const int I, const int J, const int64_t row) {
#pragma clang fp contract(off)
    constexpr int cls = PI + 2 * PJ, nc = p2_class_ncells(cls);
    const int W = 2 * a.nx - 1;
    const int I0 = I - PI, J0 = J - PJ;                         // the vertex the class tables count quads from
    double sslot[25], cslot[25], wwin[25];
    unsigned present = 0u;
#pragma unroll
    for (int e = 0; e < nc; ++e) {
        int rI[6], rJ[6];
        p2_cell_nodes(p2_class_cell(cls, e, 0), p2_class_cell(cls, e, 1), p2_class_cell(cls, e, 2) != 0, rI, rJ);
#pragma unroll
        for (int j = 0; j < 6; ++j) present |= 1u << ((rJ[j] - PJ + 2) * 5 + (rI[j] - PI + 2));
    }
#pragma unroll
    for (int s = 0; s < 25; ++s) {
        sslot[s] = 0.0; cslot[s] = 0.0;
        wwin[s] = (present & (1u << s)) ? a.w[(int64_t)(J + s / 5 - 2) * W + (I + s % 5 - 2)] : 0.0;
    }
    double vi = 0.0;
#pragma unroll
    for (int e = 0; e < nc; ++e) {
        const int li = p2_class_cell(cls, e, 3);
        int rI[6], rJ[6];                                       // the cell's nodes relative to (I0, J0)
        p2_cell_nodes(p2_class_cell(cls, e, 0), p2_class_cell(cls, e, 1), p2_class_cell(cls, e, 2) != 0, rI, rJ);
        const P2CellGeom g = elliptic_p2_cell_geom(a.nx, a.ny, I0, J0, rI, rJ);
        double wc[6];                                           // cur_weights[celldofs(cell)] (:253)
#pragma unroll
        for (int v = 0; v < 6; ++v) wc[v] = wwin[(rJ[v] - PJ + 2) * 5 + (rI[v] - PI + 2)];
        double se[6] = {0, 0, 0, 0, 0, 0}, ce[6] = {0, 0, 0, 0, 0, 0}, ve = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double xx = p2_tri_qpoint(q).xi, xy = p2_tri_qpoint(q).eta;
            const double dO = p2_tri_qpoint(q).w * fabs(g.det);
            double N[6], gx[6], gy[6];
#pragma unroll
            for (int v = 0; v < 6; ++v) {
                double rx, ry;
                p2_tri_shape_grad(v, xx, xy, N[v], rx, ry);
                gx[v] = g.i00 * rx + g.i10 * ry;                // J^-T grad_xi N_v
                gy[v] = g.i01 * rx + g.i11 * ry;
            }
            double cur_u = 0.0;                                 // function_value (:259)
#pragma unroll
            for (int v = 0; v < 6; ++v) cur_u += N[v] * wc[v];
            const double cur_u_sq = cur_u * cur_u;
#pragma unroll
            for (int v = 0; v < 6; ++v) {
                se[v] += (gx[v] * gx[li] + gy[v] * gy[li]) * dO;             // :220
                ce[v] += 3.0 * N[li] * cur_u_sq * N[v] * dO;                 // :270
            }
            ve += N[li] * (cur_u_sq * cur_u) * dO;                           // :272
        }
#pragma unroll
        for (int v = 0; v < 6; ++v) {                           // assemble! (:225, :275)
            const int s = (rJ[v] - PJ + 2) * 5 + (rI[v] - PI + 2);
            sslot[s] += se[v];
            cslot[s] += ce[v];
        }
        vi += ve;
    }
    // J = J_static + J_cube; f = J_static w + f_cube, the product summing the row in ascending column order
    int64_t p = a.rowptr[row];
    double acc = 0.0;
#pragma unroll
    for (int s = 0; s < 25; ++s)
        if (present & (1u << s)) {
            a.vals[p++] = sslot[s] + cslot[s];
            acc += sslot[s] * wwin[s];
        }
    a.f[row] = acc + vi;
}

__device__ __forceinline__ void elliptic_p2_row(const EllipticP2Args& a, const int64_t row) {
    const int W = 2 * a.nx - 1, H = 2 * a.ny - 1;
    if (row >= (int64_t)W * H) return;
    const int I = (int)(row % W), J = (int)(row / W);
    if (I == 0 || J == 0 || I == W - 1 || J == H - 1) {        // prescribed: the row stays zero
        for (int64_t p = a.rowptr[row]; p < a.rowptr[row + 1]; ++p) a.vals[p] = 0.0;
        a.f[row] = 0.0;
        return;
    }
    switch ((I & 1) + 2 * (J & 1)) {
        case 0: elliptic_p2_row_class<0, 0>(a, I, J, row); break;
        case 1: elliptic_p2_row_class<1, 0>(a, I, J, row); break;
        case 2: elliptic_p2_row_class<0, 1>(a, I, J, row); break;
        default: elliptic_p2_row_class<1, 1>(a, I, J, row); break;
    }
}

// A batch of linearisation points on one mesh, problem-major: w[B][n] -> vals[B][nnz], f[B][n]; blockIdx.y is the problem
// (a one-problem call is a batch of 1).  A row's arithmetic does not depend on the problem's place in the batch.
__global__ __launch_bounds__(256) void elliptic_p2_rows_batch(EllipticP2Args a, int64_t nnz) {
    const int64_t p = blockIdx.y, n = (int64_t)(2 * a.nx - 1) * (2 * a.ny - 1);
    a.w += p * n; a.vals += p * nnz; a.f += p * n;
    elliptic_p2_row(a, (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
}

// b[i] = sum_cells sum_q N_i(xi_q) src_q[cell][q] dOmega over the point's cells (:222); prescribed rows stay zero
template <int PI, int PJ>
__device__ __forceinline__ double elliptic_p2_load_class(const EllipticP2LoadArgs& a, const int I, const int J) {
#pragma clang fp contract(off)
    constexpr int cls = PI + 2 * PJ, nc = p2_class_ncells(cls);
    const int I0 = I - PI, J0 = J - PJ;
    const int64_t nlow = (int64_t)(a.nx - 1) * (a.ny - 1);
    double bi = 0.0;
#pragma unroll
    for (int e = 0; e < nc; ++e) {
        const int dqx = p2_class_cell(cls, e, 0), dqy = p2_class_cell(cls, e, 1), li = p2_class_cell(cls, e, 3);
        const bool upper = p2_class_cell(cls, e, 2) != 0;
        int rI[6], rJ[6];
        p2_cell_nodes(dqx, dqy, upper, rI, rJ);
        const P2CellGeom g = elliptic_p2_cell_geom(a.nx, a.ny, I0, J0, rI, rJ);
        const int64_t cell = (upper ? nlow : 0) + (int64_t)(J0 / 2 + dqy) * (a.nx - 1) + (I0 / 2 + dqx);
        double fe = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            double Ni, rx, ry;
            p2_tri_shape_grad(li, p2_tri_qpoint(q).xi, p2_tri_qpoint(q).eta, Ni, rx, ry);
            fe += Ni * a.src[cell * 4 + q] * (p2_tri_qpoint(q).w * fabs(g.det));
        }
        bi += fe;
    }
    return bi;
}

__device__ __forceinline__ void elliptic_p2_load_row(const EllipticP2LoadArgs& a, const int64_t row) {
    const int W = 2 * a.nx - 1, H = 2 * a.ny - 1;
    if (row >= (int64_t)W * H) return;
    const int I = (int)(row % W), J = (int)(row / W);
    if (I == 0 || J == 0 || I == W - 1 || J == H - 1) { a.b[row] = 0.0; return; }
    double bi;
    switch ((I & 1) + 2 * (J & 1)) {
        case 0: bi = elliptic_p2_load_class<0, 0>(a, I, J); break;
        case 1: bi = elliptic_p2_load_class<1, 0>(a, I, J); break;
        case 2: bi = elliptic_p2_load_class<0, 1>(a, I, J); break;
        default: bi = elliptic_p2_load_class<1, 1>(a, I, J); break;
    }
    a.b[row] = bi;
}

// src[B][cells][4] -> b[B][n]; blockIdx.y is the problem (B = 1: the one-problem call)
__global__ __launch_bounds__(256) void elliptic_p2_load_batch(EllipticP2LoadArgs a) {
    const int64_t p = blockIdx.y, n = (int64_t)(2 * a.nx - 1) * (2 * a.ny - 1);
    a.src += p * (8 * (int64_t)(a.nx - 1) * (a.ny - 1)); a.b += p * n;
    elliptic_p2_load_row(a, (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
}

}  // namespace gmrf
