"""NumPy restatement of the three functions the reference's nonlinear elliptic benchmark evaluates per Gauss-Newton iteration
(/root/reference/_research/elliptic_chen24.jl: `assemble_J_diff_and_f` :179-228, `assemble_J_cube` :231-278, `f_and_J`
:280-285) on the structured P1 triangle mesh, written cell by cell with Ferrite's reference triangle, plus the loops of
tests/gn_batch_oracle.py around them.  Not a test module.

Mesh: nx x ny nodes on the unit square, x fastest; every quad is cut by the diagonal n00 - n11 into the cells (n00, n10, n11)
[all of them first] and (n00, n11, n01).  Element: Lagrange{RefTriangle,1} with the vertices (1,0), (0,1), (0,0), N = (xi, eta,
1 - xi - eta); QuadratureRule{RefTriangle}(2): the points (1/6,1/6), (1/6,2/3), (2/3,1/6) with weight 1/6 each."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from oracle import bt_oracle as O
from tests import gn_batch_oracle as GO

QP = ((1 / 6, 1 / 6), (1 / 6, 2 / 3), (2 / 3, 1 / 6))
QW = 1 / 6
DN_REF = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, -1.0]])          # dN_v / d(xi, eta)


class Mesh:
    def __init__(self, nx: int, ny: int):
        self.nx, self.ny, self.n = nx, ny, nx * ny
        xs, ys = np.linspace(0.0, 1.0, nx), np.linspace(0.0, 1.0, ny)
        self.coords = np.array([(xs[i % nx], ys[i // nx]) for i in range(self.n)])
        lower, upper = [], []
        for qy in range(ny - 1):
            for qx in range(nx - 1):
                n00 = qy * nx + qx
                n10, n01, n11 = n00 + 1, n00 + nx, n00 + nx + 1
                lower.append((n00, n10, n11)); upper.append((n00, n11, n01))
        self.cells = lower + upper
        ix, iy = np.arange(self.n) % nx, np.arange(self.n) // nx
        self.prescribed = set(np.flatnonzero((ix == 0) | (iy == 0) | (ix == nx - 1) | (iy == ny - 1)).tolist())
        # allocate_matrix(dh, ch): every pair of dofs that share a cell
        rows = np.array([c[i] for c in self.cells for i in range(3) for _ in range(3)])
        cols = np.array([c[j] for c in self.cells for _ in range(3) for j in range(3)])
        P = sp.coo_matrix((np.ones(rows.size), (rows, cols)), shape=(self.n, self.n)).tocsr()
        P.sort_indices()
        P.data[:] = 1.0
        self.pattern = P
        self.pos = {}
        for i in range(self.n):
            for k in range(P.indptr[i], P.indptr[i + 1]):
                self.pos[(i, int(P.indices[k]))] = k

    def cellvalues(self, cell):
        """reinit!(cellvalues, cell): per quadrature point (dOmega, N, dN/dx, x_q)."""
        X = self.coords[list(cell)]                                # (3, 2)
        Jm = X.T @ DN_REF                                          # dx / dxi
        det = Jm[0, 0] * Jm[1, 1] - Jm[0, 1] * Jm[1, 0]
        dN = DN_REF @ np.linalg.inv(Jm)                            # physical gradients (constant on a P1 cell)
        out = []
        for xi, eta in QP:
            N = np.array([xi, eta, 1.0 - xi - eta])
            out.append((abs(det) * QW, N, dN, N @ X))
        return out

    def matrix(self, vals):
        return sp.csr_matrix((np.asarray(vals, dtype=np.float64), self.pattern.indices, self.pattern.indptr), shape=(self.n, self.n))


def qpoints(mesh: Mesh) -> np.ndarray:
    """spatial_coordinate(cellvalues, q_point, cell_coords) (:206) of every cell: (cells, 3, 2)."""
    return np.array([[cv[3] for cv in mesh.cellvalues(c)] for c in mesh.cells])


def assemble_J_diff_and_f(mesh: Mesh, rhs_q):
    """:179-228.  rhs_q[cell][q] = rhs_fn(x_q).  Returns (values of J_diff on mesh.pattern, f)."""
    vals, f = np.zeros(mesh.pattern.nnz), np.zeros(mesh.n)
    for ci, cell in enumerate(mesh.cells):                         # CellIterator(dh)
        Je, fe = np.zeros((3, 3)), np.zeros(3)
        for q, (dO, N, dN, _) in enumerate(mesh.cellvalues(cell)):     # :203
            rhs_val = rhs_q[ci][q]                                 # :207
            for i in range(3):
                if cell[i] in mesh.prescribed:                     # :210-212
                    continue
                for j in range(3):
                    Je[i, j] += (dN[j] @ dN[i]) * dO               # :220
                fe[i] += N[i] * rhs_val * dO                       # :222
        for i in range(3):                                         # assemble! :225
            for j in range(3):
                vals[mesh.pos[(cell[i], cell[j])]] += Je[i, j]
            f[cell[i]] += fe[i]
    return vals, f


def assemble_J_cube(mesh: Mesh, cur_weights):
    """:231-278.  Returns (values of J_cube on mesh.pattern, v)."""
    vals, v = np.zeros(mesh.pattern.nnz), np.zeros(mesh.n)
    for cell in mesh.cells:
        Je, ve = np.zeros((3, 3)), np.zeros(3)
        w = np.array([cur_weights[d] for d in cell])               # :253
        for dO, N, _, _ in mesh.cellvalues(cell):
            cur_u = float(N @ w)                                   # :259
            cur_u_sq = cur_u * cur_u
            for i in range(3):
                if cell[i] in mesh.prescribed:                     # :262-264
                    continue
                for j in range(3):
                    Je[i, j] += 3 * N[i] * cur_u_sq * N[j] * dO    # :270
                ve[i] += N[i] * (cur_u * cur_u * cur_u) * dO       # :272
        for i in range(3):                                         # assemble! :275
            for j in range(3):
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


def single_loop(fJ, Q, Qx_prior, x_prior, x0, noise, n_blocks, rtol, max_steps):
    """The loop of gmrf_fem_solve (:148-161) for ONE problem with zero observations, under the stop rule of
    scripts/solve_burger.jl:161 / :171 (the shape of GO.single_loop).  Returns (x, steps, objective history, iterates)."""
    x = np.array(x0, dtype=np.float64)
    f, _ = fJ(x)
    obs_diff = -f
    last, cur = np.inf, GO.objective(Q, x_prior, x, obs_diff, noise)
    hist, iterates, steps = [cur], [], 0
    while GO.rel_diff(last, cur) > rtol and steps < max_steps:
        _, J = fJ(x)
        x = O.gn_step(Q, J, Qx_prior, x, obs_diff, noise, n_blocks)
        f, _ = fJ(x)
        obs_diff = -f
        last, cur = cur, GO.objective(Q, x_prior, x, obs_diff, noise)
        hist.append(cur); iterates.append(x.copy()); steps += 1
    return x, steps, np.array(hist), iterates


def batch_loop(fJs, pattern, q_values, Qx_prior, x_prior, x0, noise, n_blocks, rtol, max_steps):
    """B problems in lock step as the device driver runs them (the shape of GO.batch_loop; fJs[p] is problem p's f_and_J).
    Returns (x, steps, history padded with NaN, the tested ratios, iterates per iteration)."""
    B = x0.shape[0]
    Qs = [GO.problem_matrix(pattern, q_values if np.ndim(q_values) == 1 else q_values[p]) for p in range(B)]
    x = np.array(x0, dtype=np.float64)
    obs = np.empty_like(x)
    last, cur = np.full(B, np.inf), np.empty(B)
    steps = np.zeros(B, dtype=np.int32)
    hist = np.full((B, max_steps + 1), np.nan)
    rels = np.full((B, max_steps + 1), np.nan)
    for p in range(B):
        f, _ = fJs[p](x[p])
        obs[p] = -f
        cur[p] = hist[p, 0] = GO.objective(Qs[p], x_prior[p], x[p], obs[p], noise)
        rels[p, 0] = GO.rel_diff(last[p], cur[p])
    active = np.array([rels[p, 0] > rtol and 0 < max_steps for p in range(B)])
    iterates = []
    while active.any():
        for p in range(B):
            if not active[p]:                                      # (frozen: the device solves it again and drops the result)
                continue
            _, J = fJs[p](x[p])
            cand = O.gn_step(Qs[p], J, Qx_prior[p], x[p], obs[p], noise, n_blocks)
            f, _ = fJs[p](cand)
            x[p], obs[p] = cand, -f
            last[p], cur[p] = cur[p], GO.objective(Qs[p], x_prior[p], cand, obs[p], noise)
            steps[p] += 1
            hist[p, steps[p]] = cur[p]
            rels[p, steps[p]] = GO.rel_diff(last[p], cur[p])
            active[p] = rels[p, steps[p]] > rtol and steps[p] < max_steps
        iterates.append(x.copy())
    return x, steps, hist, rels, iterates


# The case tests/test_gpu_elliptic.py runs against `batch_loop`, on both meshes; tests/test_elliptic_cpu.py checks with the
# oracle alone that its stop decisions are far from the threshold and that its problems stop at different counts.
GN_CASE = {"meshes": ((16, 16), (19, 14)), "amps": (0.0, 0.5, 1.0, 2.0), "B": 4, "rows_per_block": 2, "rtol": 1e-5, "max_steps": 10}


def oracle_case(workloads, mesh_size, case=GN_CASE, max_steps=None):
    """(workload dict, Problem, batch_loop result) of GN_CASE on one mesh."""
    w = workloads.elliptic_gauss_newton_batch(mesh_size, case["B"], rows_per_block=case["rows_per_block"], amps=case["amps"])
    prob = Problem(w["nx"], w["ny"], w["src_q"])
    res = batch_loop([prob.fJ(p) for p in range(case["B"])], w["Q"], w["q_values"], w["Qx_prior"], w["x_prior"], w["x0"], w["noise"],
                     w["n_blocks"], case["rtol"], case["max_steps"] if max_steps is None else max_steps)
    return w, prob, res
