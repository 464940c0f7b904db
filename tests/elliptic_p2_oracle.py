"""NumPy restatement of the three functions the reference's nonlinear elliptic benchmark evaluates per Gauss-Newton iteration
(_research/elliptic_chen24.jl of the reference: `assemble_J_diff_and_f` :179-228, `assemble_J_cube` :231-278, `f_and_J`
:280-285) with the reference's default element (`element_order = 2`, :118-122), written cell by cell on the structured
quadratic mesh of the oracle.  The shape of tests/elliptic_oracle.py, whose loops serve both orders.  Not a test module.

Mesh: `O.p2_lattice_cells` -- the P1 triangulation of nx x ny vertices, every cell with its three edge midpoints; dofs are the
points of the (2 nx - 1) x (2 ny - 1) lattice, x fastest.  Element: Lagrange{RefTriangle,2} (`O._p2_triangle_shape`,
`O._p2_triangle_ref_grad`: vertices at (1,0), (0,1), (0,0), then the nodes of the edges (1-2), (2-3), (3-1));
QuadratureRule{RefTriangle}(3): `O.P2_TRI_QPOINTS`, whose order fixes every sum over quadrature points."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from oracle import bt_oracle as O
from tests.elliptic_oracle import batch_loop, single_loop          # noqa: F401  (the loops do not know the element)

NQ = len(O.P2_TRI_QPOINTS)


class Mesh:
    def __init__(self, nx: int, ny: int):
        self.nx, self.ny = nx, ny
        self.W, self.H = 2 * nx - 1, 2 * ny - 1
        self.n = self.W * self.H
        cells, X, Y = O.p2_lattice_cells(nx, ny)
        self.cells = [tuple(int(d) for d in c) for c in cells]
        self.vx, self.vy = X, Y                                    # (cells, 3) vertex coordinates
        xs, ys = np.linspace(0.0, 1.0, nx), np.linspace(0.0, 1.0, ny)
        I, J = np.arange(self.n) % self.W, np.arange(self.n) // self.W
        self.coords = np.stack([0.5 * (xs[I // 2] + xs[(I + 1) // 2]), 0.5 * (ys[J // 2] + ys[(J + 1) // 2])], axis=1)
        self.prescribed = set(np.flatnonzero((I == 0) | (J == 0) | (I == self.W - 1) | (J == self.H - 1)).tolist())
        # allocate_matrix(dh, ch): every pair of dofs that share a cell
        rows = np.array([c[i] for c in self.cells for i in range(6) for _ in range(6)])
        cols = np.array([c[j] for c in self.cells for _ in range(6) for j in range(6)])
        P = sp.coo_matrix((np.ones(rows.size), (rows, cols)), shape=(self.n, self.n)).tocsr()
        P.sort_indices()
        P.data[:] = 1.0
        self.pattern = P
        self.pos = {}
        for i in range(self.n):
            for k in range(P.indptr[i], P.indptr[i + 1]):
                self.pos[(i, int(P.indices[k]))] = k
        self._cv = [self._cellvalues(ci) for ci in range(len(self.cells))]

    def _cellvalues(self, ci):
        x, y = self.vx[ci], self.vy[ci]
        a, b, c, d = x[0] - x[2], x[1] - x[2], y[0] - y[2], y[1] - y[2]      # J = [[a, b], [c, d]] = [x_1 - x_3, x_2 - x_3]
        det = a * d - b * c
        out = []
        for xi, eta, wq in O.P2_TRI_QPOINTS:
            g = 1.0 - xi - eta
            N = O._p2_triangle_shape(xi, eta)
            r = O._p2_triangle_ref_grad(xi, eta)
            dN = np.stack([(d * r[:, 0] - c * r[:, 1]) / det, (-b * r[:, 0] + a * r[:, 1]) / det], axis=1)      # J^-T grad_xi
            xq = np.array([(xi * x[0] + eta * x[1]) + g * x[2], (xi * y[0] + eta * y[1]) + g * y[2]])
            out.append((wq * abs(det), N, dN, xq))
        return out

    def cellvalues(self, ci):
        """reinit!(cellvalues, cell): per quadrature point (dOmega, N, dN/dx, x_q)."""
        return self._cv[ci]

    def matrix(self, vals):
        return sp.csr_matrix((np.asarray(vals, dtype=np.float64), self.pattern.indices, self.pattern.indptr), shape=(self.n, self.n))


def qpoints(mesh: Mesh) -> np.ndarray:
    """spatial_coordinate(cellvalues, q_point, cell_coords) (:206) of every cell: (cells, 4, 2)."""
    return np.array([[cv[3] for cv in mesh.cellvalues(ci)] for ci in range(len(mesh.cells))])


def assemble_J_diff_and_f(mesh: Mesh, rhs_q, mask_rows: bool = True):
    """:179-228.  rhs_q[cell][q] = rhs_fn(x_q).  Returns (values of J_diff on mesh.pattern, f).  mask_rows = False keeps the
    rows of prescribed dofs (to compare the element sums with the Darcy P2 restatement)."""
    vals, f = np.zeros(mesh.pattern.nnz), np.zeros(mesh.n)
    for ci, cell in enumerate(mesh.cells):                         # CellIterator(dh)
        Je, fe = np.zeros((6, 6)), np.zeros(6)
        for q, (dO, N, dN, _) in enumerate(mesh.cellvalues(ci)):   # :203
            rhs_val = rhs_q[ci][q]                                 # :207
            for i in range(6):
                if mask_rows and cell[i] in mesh.prescribed:       # :210-212
                    continue
                for j in range(6):
                    Je[i, j] += (dN[j, 0] * dN[i, 0] + dN[j, 1] * dN[i, 1]) * dO      # :220
                fe[i] += N[i] * rhs_val * dO                       # :222
        for i in range(6):                                         # assemble! :225
            for j in range(6):
                vals[mesh.pos[(cell[i], cell[j])]] += Je[i, j]
            f[cell[i]] += fe[i]
    return vals, f


def assemble_J_cube(mesh: Mesh, cur_weights):
    """:231-278.  Returns (values of J_cube on mesh.pattern, v)."""
    vals, v = np.zeros(mesh.pattern.nnz), np.zeros(mesh.n)
    for ci, cell in enumerate(mesh.cells):
        Je, ve = np.zeros((6, 6)), np.zeros(6)
        w = [float(cur_weights[d]) for d in cell]                  # :253
        for dO, N, _, _ in mesh.cellvalues(ci):
            cur_u = 0.0                                            # :259
            for k in range(6):
                cur_u += float(N[k]) * w[k]
            cur_u_sq = cur_u * cur_u
            for i in range(6):
                if cell[i] in mesh.prescribed:                     # :262-264
                    continue
                for j in range(6):
                    Je[i, j] += 3 * N[i] * cur_u_sq * N[j] * dO    # :270
                ve[i] += N[i] * (cur_u_sq * cur_u) * dO            # :272
        for i in range(6):                                         # assemble! :275
            for j in range(6):
                vals[mesh.pos[(cell[i], cell[j])]] += Je[i, j]
            v[cell[i]] += ve[i]
    return vals, v


def f_and_J(w, mesh: Mesh, J_static_vals, f_static):
    """:280-285.  Returns (f, J as CSR on mesh.pattern)."""
    cube_vals, f_cube = assemble_J_cube(mesh, w)
    f = mesh.matrix(J_static_vals) @ w + f_cube - f_static
    return f, mesh.matrix(J_static_vals + cube_vals)


class Problem:
    """One mesh with its static part; `fJ(p)` is the closure the loops call for problem p of a batch of sources."""

    def __init__(self, nx, ny, src_q):
        self.mesh = Mesh(nx, ny)
        src_q = np.asarray(src_q, dtype=np.float64)
        self.src_q = src_q if src_q.ndim == 3 else src_q[None]
        parts = [assemble_J_diff_and_f(self.mesh, s) for s in self.src_q]
        self.J_static = parts[0][0]
        self.f_static = np.stack([p[1] for p in parts])

    def fJ(self, p):
        return lambda x: f_and_J(x, self.mesh, self.J_static, self.f_static[p])


# The case tests/test_gpu_elliptic_p2.py runs against `batch_loop`, on both meshes (vertices per side): the lattices are 15 x 15 =
# 225 dofs (3 blocks of 75) and 19 x 15 = 285 dofs (3 blocks of 95; non-square, the last workgroup partial).
# tests/test_elliptic_p2_cpu.py checks with the oracle alone that its stop decisions are far from the threshold and that its
# problems stop at different counts.
GN_CASE_P2 = {"meshes": ((8, 8), (10, 8)), "amps": (0.0, 0.25, 1.0, 2.0), "B": 4, "rows_per_block": 5, "rtol": 1e-5, "max_steps": 10}


def oracle_case(workloads, mesh_size, case=GN_CASE_P2, max_steps=None):
    """(workload dict, Problem, batch_loop result) of GN_CASE_P2 on one mesh."""
    w = workloads.elliptic_gauss_newton_batch(mesh_size, case["B"], rows_per_block=case["rows_per_block"], amps=case["amps"], order=2)
    prob = Problem(w["nx"], w["ny"], w["src_q"])
    res = batch_loop([prob.fJ(p) for p in range(case["B"])], w["Q"], w["q_values"], w["Qx_prior"], w["x_prior"], w["x0"], w["noise"],
                     w["n_blocks"], case["rtol"], case["max_steps"] if max_steps is None else max_steps)
    return w, prob, res
