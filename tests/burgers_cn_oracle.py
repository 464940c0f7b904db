"""NumPy restatement of the Burgers line tangent over (order, scheme, bc) -- gmrf_burgers_line_create -- and of the batched
Gauss-Newton loop on it, on SuperLU.  Written from the element loops of the reference (src/problems/burgers.jl:22-51 the
advection tangent and residual, :60-98 mass and stiffness, :53-57 / :87-92 the prescribed dofs) and its two time schemes
(scripts/burgers/solve_burgers_gmrf-fem.jl:118-149 implicit Euler; _research/burgers_chen24.jl:121-132, :195-226
Crank-Nicolson), vectorised over the cells.  Not a test module.

Row block of the step t-1 -> t (t = 1 .. nt-1, 0-based), M / G consistent mass and stiffness, A(w) / v(w) advection tangent and
residual of one slice:
    euler  J[:, t-1] = -M                                     J[:, t] = M + dt nu G + dt A(w_t)             f += dt v(w_t)
    cn     J[:, t-1] = -M + dt nu 0.5 G + dt 0.5 A(w_{t-1})   J[:, t] = M + dt nu 0.5 G + dt 0.5 A(w_t)     f += dt 0.5 (v(w_{t-1}) + v(w_t))
with f = (J without its A terms) w + the advection part.  Dirichlet: dofs 0 and ns-1 are prescribed; their rows and columns of M,
G, A and their entries of v are zero, and they stay in the system as stored zeros."""
from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests import gn_batch_oracle as GO

_XI = (-np.sqrt(3.0 / 5.0), 0.0, np.sqrt(3.0 / 5.0))       # QuadratureRule{RefLine}(3)
_WQ = (5.0 / 9.0, 8.0 / 9.0, 5.0 / 9.0)


def cell_values(h: float, order: int):
    """Per quadrature point (detJ dV, shape values, physical shape gradients) of one cell of length h; quadratic cells in Ferrite's
    local order (left, right, middle)."""
    jac = 0.5 * h
    out = []
    for x, wq in zip(_XI, _WQ):
        if order == 1:
            N, dN = (0.5 * (1.0 - x), 0.5 * (1.0 + x)), (-0.5 / jac, 0.5 / jac)
        else:
            N = (0.5 * x * (x - 1.0), 0.5 * x * (x + 1.0), 1.0 - x * x)
            dN = ((x - 0.5) / jac, (x + 0.5) / jac, (-2.0 * x) / jac)
        out.append((jac * wq, N, dN))
    return out


class Line:
    """nc cells of the order-1 or order-2 line, periodic (order nc dofs, wrap-around) or dirichlet (order nc + 1 dofs, the two
    ends prescribed), dofs numbered by position.  Holds the spatial coupling pattern (CSR, sorted), the place of every
    element-matrix entry in it, and the assembled M and G (prescribed rows and columns zeroed)."""

    def __init__(self, nc: int, order: int, bc: str, length: float):
        if order not in (1, 2) or bc not in ("periodic", "dirichlet"):
            raise ValueError("order 1 or 2, bc periodic or dirichlet")
        self.nc, self.order, self.bc, self.nb = nc, order, bc, order + 1
        self.ns = ns = order * nc + (1 if bc == "dirichlet" else 0)
        self.h = length / nc
        e = np.arange(nc)
        cols = [order * e, order * e + order] + ([order * e + 1] if order == 2 else [])
        self.cells = np.stack(cols, axis=1) % ns if bc == "periodic" else np.stack(cols, axis=1)
        self.prescribed = np.array([0, ns - 1]) if bc == "dirichlet" else np.array([], dtype=np.int64)
        I = np.repeat(self.cells, self.nb, axis=1).ravel()          # (cell, i, j) -> dof of i
        J = np.tile(self.cells, (1, self.nb)).ravel()               # ... of j
        S = sp.coo_matrix((np.ones(I.size), (I, J)), shape=(ns, ns)).tocsr()
        S.sort_indices()
        self.indptr, self.indices, self.nnz = S.indptr.astype(np.int64), S.indices.astype(np.int64), int(S.nnz)
        look = np.full((ns, ns), -1, dtype=np.int64)
        rows = np.repeat(np.arange(ns), np.diff(self.indptr))
        look[rows, self.indices] = np.arange(self.nnz)
        self.pos = look[I, J]
        self.keep = ~(np.isin(rows, self.prescribed) | np.isin(self.indices, self.prescribed))
        self.cv = cell_values(self.h, order)
        Me, Ge = np.zeros((self.nb, self.nb)), np.zeros((self.nb, self.nb))
        for dOm, N, dN in self.cv:                                  # assemble_mass_matrix / assemble_diffusion_matrix
            for i in range(self.nb):
                for j in range(self.nb):
                    Me[i, j] += N[i] * N[j] * dOm
                    Ge[i, j] += dN[i] * dN[j] * dOm
        self.M = self.scatter(np.tile(Me.ravel(), nc))
        self.G = self.scatter(np.tile(Ge.ravel(), nc))

    def scatter(self, elem):
        """assemble! of per-cell matrices (nc nb nb values), then the zeroing of the prescribed rows and columns."""
        return np.bincount(self.pos, weights=np.ravel(elem), minlength=self.nnz) * self.keep

    def advection(self, w):
        """assemble_burgers_advection_matrix at the slice w (ns,): (A values on the pattern, v)."""
        nb, wc = self.nb, np.asarray(w, dtype=np.float64)[self.cells]
        Ge, ve = np.zeros((self.nc, nb, nb)), np.zeros((self.nc, nb))
        for dOm, N, dN in self.cv:
            cur_u, grad_u = np.zeros(self.nc), np.zeros(self.nc)
            for k in range(nb):
                cur_u += N[k] * wc[:, k]
            for k in range(nb):
                grad_u += dN[k] * wc[:, k]
            for i in range(nb):
                for j in range(nb):
                    Ge[:, i, j] += N[i] * (N[j] * grad_u + cur_u * dN[j]) * dOm
                ve[:, i] += N[i] * cur_u * grad_u * dOm
        v = np.bincount(self.cells.ravel(), weights=ve.ravel(), minlength=self.ns)
        v[self.prescribed] = 0.0
        return self.scatter(Ge), v

    def matvec(self, data, x):
        return sp.csr_matrix((data, self.indices, self.indptr), shape=(self.ns, self.ns)) @ x


@functools.lru_cache(maxsize=None)
def line(nc: int, order: int, bc: str, length: float) -> Line:
    return Line(nc, order, bc, float(length))


def f_and_J(nc, nt, dt, nu, w, order=1, scheme="euler", bc="periodic", length=1.0):
    """(f, J): J as CSR ((nt-1) ns x nt ns) with sorted indices and its explicit zeros kept: row (t, i) holds the spatial pattern's
    row i for slice t-1, then for slice t."""
    if scheme not in ("euler", "cn"):
        raise ValueError("scheme euler or cn")
    L = line(nc, order, bc, length)
    ns, nnz = L.ns, L.nnz
    W = np.asarray(w, dtype=np.float64).reshape(nt, ns)
    adv = [L.advection(W[t]) if (t > 0 or scheme == "cn") else None for t in range(nt)]
    cnt = np.diff(L.indptr)
    row_of = np.repeat(np.arange(ns), cnt)
    off = np.arange(nnz) - L.indptr[row_of]
    place_prev = 2 * L.indptr[row_of] + off                         # within one row block of 2 nnz values
    place_cur = place_prev + cnt[row_of]
    data = np.empty((nt - 1, 2 * nnz))
    indices = np.empty((nt - 1, 2 * nnz), dtype=np.int64)
    f = np.empty((nt - 1, ns))
    for t in range(1, nt):
        if scheme == "euler":
            sp_, st_ = -L.M, L.M + (dt * nu) * L.G
            jp, jc = sp_, st_ + dt * adv[t][0]
            fa = dt * adv[t][1]
        else:
            sp_, st_ = -L.M + (dt * nu * 0.5) * L.G, L.M + (dt * nu * 0.5) * L.G
            jp, jc = sp_ + (dt * 0.5) * adv[t - 1][0], st_ + (dt * 0.5) * adv[t][0]
            fa = (dt * 0.5) * (adv[t - 1][1] + adv[t][1])
        data[t - 1, place_prev], data[t - 1, place_cur] = jp, jc
        indices[t - 1, place_prev], indices[t - 1, place_cur] = (t - 1) * ns + L.indices, t * ns + L.indices
        f[t - 1] = L.matvec(sp_, W[t - 1]) + L.matvec(st_, W[t]) + fa
    indptr = np.concatenate([(np.arange(nt - 1)[:, None] * 2 * nnz + 2 * L.indptr[None, :-1]).ravel(), [2 * nnz * (nt - 1)]])
    J = sp.csr_matrix((data.ravel(), indices.ravel(), indptr), shape=((nt - 1) * ns, nt * ns))
    return f.ravel(), J


# ------------------------------------------------------------------------------------------ the Gauss-Newton loop on SuperLU
def posterior_matrix(Q, J, noise):
    """A = Q + noise J'J (scripts/solve_burger.jl:145) as CSC."""
    A = (sp.csc_matrix(Q) + noise * (J.T @ J)).tocsc()
    A.sort_indices()
    return A


def gn_step(Q, J, Qx_prior, x, obs_diff, noise):
    """scripts/solve_burger.jl:143-149 with SuperLU in the place of the Cholesky factor."""
    rhs = Qx_prior + noise * (J.T @ (J @ x + obs_diff))
    return spla.splu(posterior_matrix(Q, J, noise)).solve(rhs)


def logdet(A):
    """log det of a positive definite A from SuperLU's U (L has a unit diagonal)."""
    return float(np.sum(np.log(np.abs(spla.splu(sp.csc_matrix(A)).U.diagonal()))))


def batch_loop(fJ, Qs, Qx_prior, x_prior, x0, noise, rtol, max_steps, y=None):
    """B problems in lock step with the driver's stop rule and objective (gmrf_gn_run, gmrf_assemble_objective_batch): a problem
    is active while |last - cur| / |cur| > rtol and steps < max_steps; a stopped one keeps its x.  fJ(x) -> (f, J).
    Returns (x (B, n), steps (B,), history (B, max_steps + 1) padded with NaN, rel (B, max_steps + 1) the tested ratios,
    iterates: list over iterations of (B, n) arrays) -- the shape of tests/gn_batch_oracle.py::batch_loop."""
    B = x0.shape[0]
    x = np.array(x0, dtype=np.float64)
    last, cur = np.full(B, np.inf), np.empty(B)
    steps = np.zeros(B, dtype=np.int32)
    hist = np.full((B, max_steps + 1), np.nan)
    rels = np.full((B, max_steps + 1), np.nan)
    obs, Js = [None] * B, [None] * B
    for p in range(B):
        f, Js[p] = fJ(x[p])
        obs[p] = (0.0 if y is None else y[p]) - f
        cur[p] = hist[p, 0] = GO.objective(Qs[p], x_prior[p], x[p], obs[p], noise)
        rels[p, 0] = GO.rel_diff(last[p], cur[p])
    active = np.array([rels[p, 0] > rtol and 0 < max_steps for p in range(B)])
    iterates = []
    while active.any():
        for p in np.flatnonzero(active):
            cand = gn_step(Qs[p], Js[p], Qx_prior[p], x[p], obs[p], noise)
            f, Js[p] = fJ(cand)
            x[p], obs[p] = cand, (0.0 if y is None else y[p]) - f
            last[p], cur[p] = cur[p], GO.objective(Qs[p], x_prior[p], cand, obs[p], noise)
            steps[p] += 1
            hist[p, steps[p]] = cur[p]
            rels[p, steps[p]] = GO.rel_diff(last[p], cur[p])
            active[p] = rels[p, steps[p]] > rtol and steps[p] < max_steps
        iterates.append(x.copy())
    return x, steps, hist, rels, iterates


# The case of the loop tests (tests/test_burgers_cn_cpu.py on the oracle alone, tests/test_gpu_burgers_cn.py on the device): the
# benchmark at nu = 0.02 on 32 quadratic cells x 26 slices, three amplitudes; the reference's stop tolerance and step bound
# (scripts/solve_burger.jl:140, :171).
CHEN_CASE = {"nc": 32, "nt": 26, "B": 3, "nu": 0.02, "amps": (1.0, 0.5, 1.3), "order": 2, "rtol": 1e-4, "max_steps": 20}


def chen_case(workloads, scheme="cn", **over):
    """(workload, fJ, batch_loop result) of CHEN_CASE under `scheme`."""
    c = dict(CHEN_CASE, **over)
    w = workloads.burgers_chen24_batch(c["nc"], c["nt"], c["B"], c["nu"], c["amps"], order=c["order"], scheme=scheme)

    def fJ(x):
        return f_and_J(c["nc"], c["nt"], w["dt"], w["nu"], x, c["order"], scheme, "dirichlet", w["length"])

    Qs = [GO.problem_matrix(w["Q"], w["q_values"][p]) for p in range(c["B"])]
    return w, fJ, batch_loop(fJ, Qs, w["Qx_prior"], w["x_prior"], w["x0"], w["noise"], c["rtol"], c["max_steps"])


def last_slice_rel_err(w, x):
    """rel_err of every problem's last slice against the Cole-Hopf truth (src/metrics.jl:11-13)."""
    ns = w["ns"]
    last = np.asarray(x)[:, -ns:]
    return np.linalg.norm(last - w["truth"], axis=1) / np.linalg.norm(w["truth"], axis=1)
