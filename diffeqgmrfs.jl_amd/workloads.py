"""Synthetic FEM workloads for the block-tridiagonal GMRF hot path.

These generators build the *inputs* of the hot path (sparse SPD block-tridiagonal
posterior precisions and right-hand sides) for the BASELINE.json configs on
structured meshes.  The reference builds the same kind of matrices with
Ferrite/Gmsh P2 meshes and the FNO datasets, neither of which exists here
(SURVEY.md section 8d), so structured P1 meshes and a synthetic coefficient field
replace them.  Nothing in here is on the timed path.

Reference call sites the constructions follow:
  * Darcy stiffness / load:    /root/reference/src/problems/darcy.jl:27-62
  * nearest-grid-point lookup: /root/reference/src/datasets/darcy.jl:30-34
  * Matern prior hyper-params: /root/reference/scripts/darcy/solve_darcy_gmrf-fem.jl:92-98
  * observation noise Q_eps:   /root/reference/scripts/darcy/solve_darcy_gmrf-fem.jl:163
  * Burgers J_static:          /root/reference/scripts/burgers/solve_burgers_gmrf-fem.jl:118-149
  * Burgers prior parameters:  /root/reference/scripts/burgers/solve_burgers_gmrf-fem.jl:86-107
  * elliptic (Chen) setup:     /root/reference/_research/elliptic_chen24.jl:118-171,231-285
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


@dataclass
class Workload:
    """One posterior-solve problem: factor Q, solve Q mu = rhs, sample N(mu, Q^-1)."""

    name: str
    Q: sp.csc_matrix          # SPD, block tridiagonal with n_blocks blocks of size n // n_blocks
    rhs: np.ndarray           # information vector; posterior mean = Q^-1 rhs
    n_blocks: int
    meta: dict = field(default_factory=dict)

    @property
    def n(self) -> int:
        return self.Q.shape[0]

    @property
    def block_size(self) -> int:
        return self.n // self.n_blocks


# --------------------------------------------------------------------------- 2-D P1 FEM

def _grid_triangles(nx: int, ny: int):
    """Node ids of the 2*(nx-1)*(ny-1) triangles; every quad is cut by the same diagonal."""
    ix, iy = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing="xy")
    n00 = (iy * nx + ix).ravel()
    n10 = n00 + 1
    n01 = n00 + nx
    n11 = n01 + 1
    lower = np.stack([n00, n10, n11], axis=1)
    upper = np.stack([n00, n11, n01], axis=1)
    return np.concatenate([lower, upper], axis=0)


def p1_unit_square(nx: int, ny: int, coeff=None):
    """Lumped mass (diag), stiffness G and coefficient-weighted stiffness D on the unit square.

    Nodes are lexicographic with x fastest, so a block of `w` consecutive node rows is a
    contiguous index range: the ordering the block-tridiagonal partition needs.
    `coeff(xc, yc)` is evaluated at the element centroids (one-point quadrature, the P1
    analogue of the quadrature-point lookup in src/problems/darcy.jl:37-39).
    """
    tri = _grid_triangles(nx, ny)
    xs = np.linspace(0.0, 1.0, nx)
    ys = np.linspace(0.0, 1.0, ny)
    X = np.tile(xs, ny)
    Y = np.repeat(ys, nx)
    x = X[tri]
    y = Y[tri]
    # P1 gradients: grad phi_i = (b_i, c_i) / (2 area)
    b = np.stack([y[:, 1] - y[:, 2], y[:, 2] - y[:, 0], y[:, 0] - y[:, 1]], axis=1)
    c = np.stack([x[:, 2] - x[:, 1], x[:, 0] - x[:, 2], x[:, 1] - x[:, 0]], axis=1)
    area2 = x[:, 0] * b[:, 0] + x[:, 1] * b[:, 1] + x[:, 2] * b[:, 2]
    area = 0.5 * np.abs(area2)
    Ke = (b[:, :, None] * b[:, None, :] + c[:, :, None] * c[:, None, :]) / (4.0 * area[:, None, None])
    n = nx * ny
    rows = np.repeat(tri, 3, axis=1).ravel()
    cols = np.tile(tri, (1, 3)).ravel()
    G = sp.coo_matrix((Ke.ravel(), (rows, cols)), shape=(n, n)).tocsr()
    lumped = np.bincount(tri.ravel(), weights=np.repeat(area / 3.0, 3), minlength=n)
    D = None
    if coeff is not None:
        a = coeff(x.mean(axis=1), y.mean(axis=1))
        D = sp.coo_matrix(((Ke * a[:, None, None]).ravel(), (rows, cols)), shape=(n, n)).tocsr()
    return lumped, G, D, (X, Y)


def _dirichlet(D: sp.csr_matrix, f: np.ndarray, boundary: np.ndarray):
    """Zero the prescribed rows/columns and put a unit-scale value on their diagonal
    (Ferrite `apply!(G, f, ch)` semantics, src/problems/darcy.jl:61)."""
    keep = np.ones(D.shape[0])
    keep[boundary] = 0.0
    P = sp.diags(keep)
    scale = float(np.mean(D.diagonal()))
    Dd = (P @ D @ P + sp.diags((1.0 - keep) * scale)).tocsr()
    fd = f * keep
    return Dd, fd


def darcy_coefficient(seed: int = 523802340, n_grid: int = 241, n_modes: int = 16):
    """Piecewise-constant a(x) in {3, 12}: a smooth random Fourier field thresholded at 0,
    tabulated on the 241x241 grid of the FNO Darcy dataset (src/datasets/darcy.jl:12-13)
    and looked up nearest-neighbour like get_xy_idcs (src/datasets/darcy.jl:30-34).
    The seed is the one the reference script uses (solve_darcy_gmrf-fem.jl:55)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    kx = rng.integers(1, 6, n_modes)
    ky = rng.integers(1, 6, n_modes)
    amp = rng.standard_normal(n_modes)
    ph = rng.uniform(0, 2 * np.pi, n_modes)
    g = np.linspace(0.0, 1.0, n_grid)
    gx, gy = np.meshgrid(g, g, indexing="ij")
    fld = np.zeros_like(gx)
    for m in range(n_modes):
        fld += amp[m] * np.cos(np.pi * (kx[m] * gx + ky[m] * gy) + ph[m])
    table = np.where(fld > 0.0, 12.0, 3.0)

    def coeff(xc, yc):
        i = np.clip(np.rint(xc * (n_grid - 1)).astype(np.int64), 0, n_grid - 1)
        j = np.clip(np.rint(yc * (n_grid - 1)).astype(np.int64), 0, n_grid - 1)
        return table[i, j]

    return coeff


def matern_precision_2d(lumped, G, kappa: float, alpha: int):
    """Q_alpha = tau^2 K (C^-1 K)^(alpha-1), K = kappa^2 C + G, scaled to unit marginal variance
    (Lindgren et al. SPDE construction; what MaternSPDE{2} + discretize produce in the
    reference, scripts/darcy/solve_darcy_gmrf-fem.jl:92-98)."""
    C = sp.diags(lumped)
    Ci = sp.diags(1.0 / lumped)
    K = (kappa ** 2) * C + G
    Q = K
    for _ in range(alpha - 1):
        Q = K @ Ci @ Q
    nu = alpha - 1.0  # d = 2
    tau2 = math.gamma(nu) / (math.gamma(alpha) * 4.0 * math.pi * kappa ** (2.0 * nu))
    Q = (tau2 * Q).tocsr()
    return ((Q + Q.T) * 0.5).tocsr()


def darcy(n_xy: int, rows_per_block: int = 4, q_eps: float = 1e8, beta: float = 1.0,
          seed: int = 523802340) -> Workload:
    """2-D Darcy posterior precision Q_post = Q_matern(alpha=3) + q_eps D^T D and the
    information vector rhs = q_eps D^T f (prior mean zero).

    Mirrors scripts/darcy/solve_darcy_gmrf-fem.jl:176-192: `condition_on_observations(x, A=D,
    Q_eps, y=f)` followed by mean / rand / std.
    """
    assert n_xy % rows_per_block == 0
    coeff = darcy_coefficient(seed)
    lumped, G, D, (X, Y) = p1_unit_square(n_xy, n_xy, coeff)
    rng_range = 1.0 / math.sqrt(n_xy)            # script :98
    kappa = math.sqrt(8.0 * 2.0) / rng_range     # smoothness 2
    Q0 = matern_precision_2d(lumped, G, kappa, alpha=3)
    f = beta * lumped.copy()                      # f_i = beta * int phi_i
    on_bnd = (X == 0.0) | (X == 1.0) | (Y == 0.0) | (Y == 1.0)
    Dd, fd = _dirichlet(D, f, np.flatnonzero(on_bnd))
    Q = (Q0 + q_eps * (Dd.T @ Dd)).tocsc()
    Q = ((Q + Q.T) * 0.5).tocsc()
    Q.sort_indices()
    rhs = q_eps * (Dd.T @ fd)
    return Workload(f"darcy{n_xy}", Q, np.asarray(rhs), n_xy // rows_per_block,
                    {"kappa": kappa, "q_eps": q_eps, "rows_per_block": rows_per_block,
                     "nnz": int(Q.nnz), "mesh": f"{n_xy}x{n_xy} P1"})


def darcy_conditioning(n_xy: int, rows_per_block: int = 4, q_eps: float = 1e8, beta: float = 1.0,
                       seeds=(523802340,)):
    """The ingredients of the reference's Darcy problem loop (scripts/darcy/solve_darcy_gmrf-fem.jl:
    176-192) on the mesh of `darcy`: the Matern prior precision Q0 (mean zero), and per seed the
    observation pair (A = Dirichlet-modified Darcy stiffness for that coefficient field, y = load) --
    all A share one sparsity pattern.  Returns (Q0, [(A, y), ...], n_blocks)."""
    obs = []
    pat = None
    for seed in seeds:
        coeff = darcy_coefficient(seed)
        lumped, G, D, (X, Y) = p1_unit_square(n_xy, n_xy, coeff)
        on_bnd = (X == 0.0) | (X == 1.0) | (Y == 0.0) | (Y == 1.0)
        Dd, fd = _dirichlet(D, beta * lumped.copy(), np.flatnonzero(on_bnd))
        if pat is None:
            pat = abs(p1_unit_square(n_xy, n_xy, lambda x, y: np.ones_like(x))[2]).tocsr() + sp.identity(n_xy * n_xy)
            pat.data[:] = 0.0
        Dd = (Dd + pat).tocsr()                   # explicit zeros: one pattern for every coefficient field
        Dd.sort_indices()
        obs.append((Dd, fd))
    kappa = math.sqrt(8.0 * 2.0) * math.sqrt(n_xy)
    lumped, G, _, _ = p1_unit_square(n_xy, n_xy)
    Q0 = matern_precision_2d(lumped, G, kappa, alpha=3).tocsc()
    Q0.sort_indices()
    return Q0, obs, n_xy // rows_per_block


def elliptic(n_xy: int, rows_per_block: int = 2, bnd_noise: float = 1e12,
             fem_noise: float = 3e13) -> Workload:
    """Nonlinear elliptic -Lap u + u^3 = f (Chen et al.) linearised at the true solution:
    Q_post = Q_matern(alpha=2, range 0.1) + bnd_noise A_b^T A_b + fem_noise J^T J with
    J = G + 3 u^2-weighted lumped mass (_research/elliptic_chen24.jl:118-171, 231-285)."""
    assert n_xy % rows_per_block == 0
    lumped, G, _, (X, Y) = p1_unit_square(n_xy, n_xy)
    kappa = math.sqrt(8.0 * 1.0) / 0.1
    Q0 = matern_precision_2d(lumped, G, kappa, alpha=2)
    u = np.sin(np.pi * X) * np.sin(np.pi * Y) + 4.0 * np.sin(4 * np.pi * X) * np.sin(4 * np.pi * Y)
    on_bnd = (X == 0.0) | (X == 1.0) | (Y == 0.0) | (Y == 1.0)
    interior = (~on_bnd).astype(np.float64)
    J = (sp.diags(interior) @ (G + sp.diags(3.0 * u * u * lumped))).tocsr()
    Ab = sp.diags(on_bnd.astype(np.float64)).tocsr()
    Q = (Q0 + bnd_noise * (Ab.T @ Ab) + fem_noise * (J.T @ J)).tocsc()
    Q = ((Q + Q.T) * 0.5).tocsc()
    Q.sort_indices()
    lap_u = 2 * np.pi ** 2 * np.sin(np.pi * X) * np.sin(np.pi * Y) \
        + 4.0 * 32 * np.pi ** 2 * np.sin(4 * np.pi * X) * np.sin(4 * np.pi * Y)
    fvals = lap_u + u ** 3
    resid = interior * lumped * fvals
    rhs = fem_noise * (J.T @ resid)
    return Workload(f"elliptic{n_xy}", Q, np.asarray(rhs), n_xy // rows_per_block,
                    {"kappa": kappa, "rows_per_block": rows_per_block, "nnz": int(Q.nnz)})


def p1_triangle_qpoints(nx: int, ny: int) -> np.ndarray:
    """(cells, 3, 2) quadrature points of the symmetric 3-point rule on the cells of `_grid_triangles` (all lower triangles,
    then all upper): point q has the barycentric weight 2/3 on cell vertex 2 - q and 1/6 on the other two -- what
    `EllipticP1Tangent.qpoints` and `ShallowWaterP1.qpoints` report."""
    tri = _grid_triangles(nx, ny)
    X = np.linspace(0.0, 1.0, nx)[tri % nx]
    Y = np.linspace(0.0, 1.0, ny)[tri // nx]
    bary = np.array([[1 / 6, 1 / 6, 2 / 3], [1 / 6, 2 / 3, 1 / 6], [2 / 3, 1 / 6, 1 / 6]])
    xq = (bary[None, :, 0] * X[:, None, 0] + bary[None, :, 1] * X[:, None, 1]) + bary[None, :, 2] * X[:, None, 2]
    yq = (bary[None, :, 0] * Y[:, None, 0] + bary[None, :, 1] * Y[:, None, 1]) + bary[None, :, 2] * Y[:, None, 2]
    return np.stack([xq, yq], axis=2)


# Lagrange{RefTriangle,2} in Ferrite's reference coordinates (vertices at xi = (1, 0), (0, 1), (0, 0), then the nodes of the edges
# (1-2), (2-3), (3-1)) and the 4-point rule of degree 3 taken for QuadratureRule{RefTriangle}(3): what csrc/fem_assemble_p2.hpp
# documents for the device and oracle/bt_oracle.py for the parity target.
_P2_TRI_RULE = ((1.0 / 3.0, 1.0 / 3.0, -27.0 / 96.0), (0.2, 0.2, 25.0 / 96.0), (0.6, 0.2, 25.0 / 96.0), (0.2, 0.6, 25.0 / 96.0))


def _p2_ref_grad(xi: float, eta: float) -> np.ndarray:
    g = 1.0 - xi - eta
    return np.array([[4.0 * xi - 1.0, 0.0], [0.0, 4.0 * eta - 1.0], [-(4.0 * g - 1.0), -(4.0 * g - 1.0)],
                     [4.0 * eta, 4.0 * xi], [-4.0 * eta, 4.0 * (g - eta)], [4.0 * (g - xi), -4.0 * xi]])


def _p2_lattice_cells(nx: int, ny: int):
    """(cells, 6) lattice dofs of the quadratic triangles on `_grid_triangles` in Ferrite's local order, and the (cells, 3)
    vertex node ids.  Dofs are the points of the (2 nx - 1) x (2 ny - 1) lattice, x fastest."""
    tri = _grid_triangles(nx, ny)
    vI, vJ = 2 * (tri % nx), 2 * (tri // nx)
    I = np.concatenate([vI, (vI + np.roll(vI, -1, axis=1)) // 2], axis=1)
    J = np.concatenate([vJ, (vJ + np.roll(vJ, -1, axis=1)) // 2], axis=1)
    return J * (2 * nx - 1) + I, tri


def p2_unit_square(nx: int, ny: int):
    """Lumped mass (diag), stiffness G and coordinates (X, Y) of quadratic triangles on the unit square: the triangulation of
    `p1_unit_square` on nx x ny vertices, dofs = the points of the (2 nx - 1) x (2 ny - 1) lattice (vertices and edge midpoints, x
    fastest), so a block of consecutive lattice rows is a contiguous index range.  G is assembled under the 4-point rule of
    degree 3 (it is `assemble_darcy_diff_matrix_p2` of the oracle with coefficient 1 and no constraints; explicit zeros kept).

    The lumped mass is the HRZ (diagonal-scaling) one: every cell gives |T| / 19 to each of its vertices and 16 |T| / 57 to each
    of its edge midpoints -- the diagonal of the consistent P2 mass (|T| / 30 and 8 |T| / 45) scaled to sum to |T|.  Row-sum
    lumping is unusable here (a P2 vertex function integrates to zero).  This is a stated deviation: the reference lumps inside
    GaussianMarkovRandomFields.jl, which is not available to compare against."""
    cells, tri = _p2_lattice_cells(nx, ny)
    xs, ys = np.linspace(0.0, 1.0, nx), np.linspace(0.0, 1.0, ny)
    Xv, Yv = xs[tri % nx], ys[tri // nx]
    a, b = Xv[:, 0] - Xv[:, 2], Xv[:, 1] - Xv[:, 2]            # J = [[a, b], [c, d]] = [x_1 - x_3, x_2 - x_3]
    c, d = Yv[:, 0] - Yv[:, 2], Yv[:, 1] - Yv[:, 2]
    det = a * d - b * c
    Ge = np.zeros((cells.shape[0], 6, 6))
    for xi, eta, wq in _P2_TRI_RULE:
        dN = _p2_ref_grad(xi, eta)
        gx = (d[:, None] * dN[None, :, 0] - c[:, None] * dN[None, :, 1]) / det[:, None]        # J^-T grad_xi
        gy = (-b[:, None] * dN[None, :, 0] + a[:, None] * dN[None, :, 1]) / det[:, None]
        Ge += (gx[:, :, None] * gx[:, None, :] + gy[:, :, None] * gy[:, None, :]) * (wq * np.abs(det))[:, None, None]
    W, H = 2 * nx - 1, 2 * ny - 1
    n = W * H
    rows = np.repeat(cells[:, :, None], 6, axis=2).ravel()
    cols = np.repeat(cells[:, None, :], 6, axis=1).ravel()
    G = sp.coo_matrix((Ge.ravel(), (rows, cols)), shape=(n, n)).tocsr()
    G.sort_indices()
    area = 0.5 * np.abs(det)
    share = np.concatenate([np.repeat((area / 19.0)[:, None], 3, axis=1), np.repeat((16.0 * area / 57.0)[:, None], 3, axis=1)], axis=1)
    lumped = np.bincount(cells.ravel(), weights=share.ravel(), minlength=n)
    I, J = np.arange(n) % W, np.arange(n) // W
    X = 0.5 * (xs[I // 2] + xs[(I + 1) // 2])
    Y = 0.5 * (ys[J // 2] + ys[(J + 1) // 2])
    return lumped, G, (X, Y)


def p2_triangle_qpoints(nx: int, ny: int) -> np.ndarray:
    """(cells, 4, 2) quadrature points of the 4-point rule of degree 3 on the cells of `_grid_triangles`:
    xi x_1 + eta x_2 + (1 - xi - eta) x_3 -- what `EllipticP1Tangent(nx, ny, order=2).qpoints` reports."""
    tri = _grid_triangles(nx, ny)
    X = np.linspace(0.0, 1.0, nx)[tri % nx]
    Y = np.linspace(0.0, 1.0, ny)[tri // nx]
    out = np.empty((tri.shape[0], 4, 2))
    for q, (xi, eta, _) in enumerate(_P2_TRI_RULE):
        g = 1.0 - xi - eta
        out[:, q, 0] = (xi * X[:, 0] + eta * X[:, 1]) + g * X[:, 2]
        out[:, q, 1] = (xi * Y[:, 0] + eta * Y[:, 1]) + g * Y[:, 2]
    return out


def _elliptic_gauss_newton_batch_p2(nx: int, ny: int, B: int, rows_per_block: int, bnd_noise: float, fem_noise: float, amps):
    """`elliptic_gauss_newton_batch` on quadratic triangles: the same dictionary on the (2 nx - 1) x (2 ny - 1) lattice.
    Dofs that share a cell are at most 2 lattice rows apart and both K C^-1 K and J'J are two hops, so the posterior reaches 4
    rows: rows_per_block >= 4 must divide the odd 2 ny - 1 (5 with ny = 3, 8, 13, ... is the smallest)."""
    W, H = 2 * nx - 1, 2 * ny - 1
    assert H % rows_per_block == 0, "rows_per_block must divide 2 ny - 1"
    lumped, G, (X, Y) = p2_unit_square(nx, ny)
    kappa = math.sqrt(8.0 * 1.0) / 0.1
    Q0 = matern_precision_2d(lumped, G, kappa, alpha=2)
    n = W * H
    I, J = np.arange(n) % W, np.arange(n) // W
    on_bnd = (I == 0) | (J == 0) | (I == W - 1) | (J == H - 1)
    Ab = sp.diags(on_bnd.astype(np.float64)).tocsr()
    Q = (Q0 + bnd_noise * (Ab.T @ Ab)).tocsc()
    Q = ((Q + Q.T) * 0.5).tocsc()
    Q.sort_indices()
    n_blocks = H // rows_per_block
    P = G.copy()
    P.data = np.ones_like(P.data)                             # the tangent's pattern: every pair of dofs that share a cell
    post = abs(Q) + (P.T @ P)
    assert block_bandwidth_ok(post, n_blocks), "Q + J'J is not block tridiagonal at this rows_per_block"
    qp = p2_triangle_qpoints(nx, ny)
    truth, src_q = np.empty((B, n)), np.empty((B,) + qp.shape[:2])
    for p in range(B):
        truth[p], _ = elliptic_truth(X, Y, amps[p])
        _, src_q[p] = elliptic_truth(qp[:, :, 0], qp[:, :, 1], amps[p])
    x_prior = np.zeros((B, n))
    return {"Q": Q, "q_values": Q.data.copy(), "x_prior": x_prior, "Qx_prior": np.zeros((B, n)), "x0": x_prior.copy(),
            "qpoints": qp, "src_q": src_q, "truth": truth, "amps": amps, "noise": fem_noise, "n_blocks": n_blocks,
            "n": n, "m": n, "nx": nx, "ny": ny, "order": 2}


def elliptic_truth(x, y, amp: float):
    """u = sin(pi x) sin(pi y) + amp sin(2 pi x) sin(2 pi y), which vanishes on the boundary of the unit square, and its
    source f_src = -Lap u + u^3.  Returns (u, f_src) at the points (x, y)."""
    s1 = np.sin(np.pi * x) * np.sin(np.pi * y)
    s2 = np.sin(2 * np.pi * x) * np.sin(2 * np.pi * y)
    u = s1 + amp * s2
    return u, 2 * np.pi ** 2 * s1 + amp * 8 * np.pi ** 2 * s2 + u ** 3


def elliptic_gauss_newton_batch(n_xy, B: int, rows_per_block: int = 2, bnd_noise: float = 1e12, fem_noise: float = 3e13,
                                amps=None, order: int = 1):
    """The ingredients of the reference's Gauss-Newton loop for -Lap u + u^3 = f (`gmrf_fem_solve`,
    _research/elliptic_chen24.jl:118-161) for B problems on one P1 mesh; n_xy: nodes per side, or (nx, ny).  Problem p has the
    true solution `elliptic_truth(., ., amps[p])` (default amps[p] = p / 2).  Returns a dict with
      Q          the prior with the boundary conditioned in, Q_matern(alpha = 2, range 0.1) + bnd_noise A_b' A_b (CSC; :125-131),
      q_values   its values (shared by every problem),
      x_prior, Qx_prior, x0   (B, n): the conditioned mean (zero: u vanishes on the boundary), Q x_prior, the start point (:148-154),
      qpoints (cells, 3, 2), src_q (B, cells, 3) the sources at the quadrature points, truth (B, n) the nodal true solutions,
      amps, noise, n_blocks, n, m, nx, ny.
    order = 2: the same on the reference's default quadratic triangles (`element_order = 2`, :118-122) -- n_xy counts vertices,
    the dofs are the (2 nx - 1) x (2 ny - 1) lattice of `p2_unit_square` (whose lumped mass is a stated deviation), qpoints
    (cells, 4, 2), src_q (B, cells, 4), n_blocks = (2 ny - 1) // rows_per_block with rows_per_block >= 4 (5 is the smallest), and
    the key "order"."""
    nx, ny = (int(n_xy), int(n_xy)) if np.ndim(n_xy) == 0 else (int(n_xy[0]), int(n_xy[1]))
    if order not in (1, 2):
        raise ValueError("order must be 1 or 2")
    if order == 2:
        amps = 0.5 * np.arange(B) if amps is None else np.asarray(amps, dtype=np.float64)
        if amps.shape != (B,):
            raise ValueError(f"amps: expected {B} amplitudes")
        return _elliptic_gauss_newton_batch_p2(nx, ny, B, rows_per_block, bnd_noise, fem_noise, amps)
    assert ny % rows_per_block == 0
    lumped, G, _, (X, Y) = p1_unit_square(nx, ny)
    kappa = math.sqrt(8.0 * 1.0) / 0.1
    Q0 = matern_precision_2d(lumped, G, kappa, alpha=2)
    on_bnd = (X == 0.0) | (X == 1.0) | (Y == 0.0) | (Y == 1.0)
    Ab = sp.diags(on_bnd.astype(np.float64)).tocsr()
    Q = (Q0 + bnd_noise * (Ab.T @ Ab)).tocsc()
    Q = ((Q + Q.T) * 0.5).tocsc()
    Q.sort_indices()
    amps = 0.5 * np.arange(B) if amps is None else np.asarray(amps, dtype=np.float64)
    if amps.shape != (B,):
        raise ValueError(f"amps: expected {B} amplitudes")
    qp = p1_triangle_qpoints(nx, ny)
    n = nx * ny
    truth, src_q = np.empty((B, n)), np.empty((B,) + qp.shape[:2])
    for p in range(B):
        truth[p], _ = elliptic_truth(X, Y, amps[p])
        _, src_q[p] = elliptic_truth(qp[:, :, 0], qp[:, :, 1], amps[p])
    x_prior = np.zeros((B, n))
    return {"Q": Q, "q_values": Q.data.copy(), "x_prior": x_prior, "Qx_prior": np.zeros((B, n)), "x0": x_prior.copy(),
            "qpoints": qp, "src_q": src_q, "truth": truth, "amps": amps, "noise": fem_noise, "n_blocks": ny // rows_per_block,
            "n": n, "m": n, "nx": nx, "ny": ny}


def elliptic_gauss_newton(n_xy, rows_per_block: int = 2, bnd_noise: float = 1e12, fem_noise: float = 3e13, amp: float = 1.0,
                          order: int = 1):
    """One problem of `elliptic_gauss_newton_batch` (its arrays without the batch axis)."""
    w = elliptic_gauss_newton_batch(n_xy, 1, rows_per_block, bnd_noise, fem_noise, amps=[amp], order=order)
    for k in ("x_prior", "Qx_prior", "x0", "src_q", "truth"):
        w[k] = w[k][0]
    w["amp"] = float(amp)
    del w["amps"]
    return w


def solution_errors(pred, soln) -> dict:
    """rmse / max_err / rel_err of an iterate against the nodal truth (/root/reference/src/metrics.jl:3-13), on the host."""
    pred, soln = np.asarray(pred, dtype=np.float64), np.asarray(soln, dtype=np.float64)
    d = pred - soln
    return {"rmse": float(np.sqrt(np.mean(d ** 2))), "max_err": float(np.max(np.abs(d))),
            "rel_err": float(np.linalg.norm(d) / np.linalg.norm(soln))}


def darcy_pred_coords(x_coords, y_coords) -> np.ndarray:
    """(len(x) len(y), 2) points of a data grid in the order of the Darcy script's `pred_coords`
    (scripts/darcy/solve_darcy_gmrf-fem.jl:82): x outer, y inner -- the `xy` of `FieldEvaluator.triangles`."""
    x, y = np.asarray(x_coords, dtype=np.float64).reshape(-1), np.asarray(y_coords, dtype=np.float64).reshape(-1)
    return np.stack([np.repeat(x, y.size), np.tile(y, x.size)], axis=1)


def burgers_pred_coords(x_coords) -> np.ndarray:
    """(len(x),) points of a data grid as the Burgers scripts' `pred_coords` (scripts/burgers/solve_burgers_gmrf-fem.jl:75) -- the
    `points` of `FieldEvaluator.line`."""
    return np.ascontiguousarray(x_coords, dtype=np.float64).reshape(-1).copy()


# --------------------------------------------------------------------------- 1-D space-time

def p1_periodic_line(ns: int):
    """Periodic P1 line on [0,1): consistent mass M, lumped mass, stiffness S, advection Adv."""
    h = 1.0 / ns
    i = np.arange(ns)
    ip = (i + 1) % ns
    im = (i - 1) % ns
    M = sp.coo_matrix((np.r_[np.full(ns, 4 * h / 6), np.full(ns, h / 6), np.full(ns, h / 6)],
                       (np.r_[i, i, i], np.r_[i, ip, im])), shape=(ns, ns)).tocsr()
    S = sp.coo_matrix((np.r_[np.full(ns, 2 / h), np.full(ns, -1 / h), np.full(ns, -1 / h)],
                       (np.r_[i, i, i], np.r_[i, ip, im])), shape=(ns, ns)).tocsr()
    Adv = sp.coo_matrix((np.r_[np.full(ns, 0.5), np.full(ns, -0.5)],
                         (np.r_[i, i], np.r_[ip, im])), shape=(ns, ns)).tocsr()
    return M, np.full(ns, h), S, Adv


def burgers_prior_from_bulk(ns: int, nt: int, bulk: float, ic, ic_noise: float = 1e8):
    """The prior part of `burgers` with the bulk speed passed in: returns (Qp, Aic, rhs) with Qp the prior precision (CSR; the
    implicit-Euler state-space blocks G x_{t+1} = M x_t + noise, G = M + dt (nu c S + gamma Adv), gamma = -c bulk, and the
    Matern(alpha=2) initial precision; scripts/burgers/solve_burgers_gmrf-fem.jl:86-107), Aic the restriction to the first
    slice and rhs = Qp (bulk 1) + ic_noise Aic' ic, the information vector of the prior conditioned on the initial condition
    (:161).  `burgers` calls it with bulk = mean(ic); the device prior (`BurgersP1Prior`) is tested against it at its own mean."""
    nu_b = 0.01 / math.pi
    dt = 1.0 / (nt - 1)
    M, lumped, S, Adv = p1_periodic_line(ns)
    ic = np.asarray(ic, dtype=np.float64)
    bulk = float(bulk)
    c = 1.0 / nu_b
    gamma = -c * bulk
    tau = 0.1 * math.sqrt(c)
    kappa = math.sqrt(8.0 * 1.5) / math.sqrt(1.0 / ns)
    Ml = sp.diags(lumped)
    K = (kappa ** 2) * Ml + S
    Q0 = (K @ sp.diags(1.0 / lumped) @ K).tocsr()
    Gm = (Ml + dt * (nu_b * c * S + gamma * Adv)).tocsr()
    W = sp.diags(np.full(ns, 1.0 / (dt * tau * tau)) / lumped)
    GWG = (Gm.T @ W @ Gm).tocsr()
    MWM = (Ml.T @ W @ Ml).tocsr()
    GWM = (Gm.T @ W @ Ml).tocsr()
    blocks = [[None] * nt for _ in range(nt)]
    for t in range(nt):
        d = GWG if t > 0 else Q0
        if t < nt - 1:
            d = d + MWM
        blocks[t][t] = d
        if t > 0:
            blocks[t][t - 1] = -GWM
            blocks[t - 1][t] = -GWM.T
    Qp = sp.bmat(blocks, format="csr")
    Aic = sp.hstack([sp.identity(ns, format="csr"), sp.csr_matrix((ns, ns * (nt - 1)))]).tocsr()
    mu0 = np.full(ns * nt, bulk)
    rhs = Qp @ mu0 + ic_noise * (Aic.T @ ic)
    return Qp, Aic, np.asarray(rhs)


def line_operators(nc: int, order: int = 1, bc: str = "periodic", length: float = 1.0):
    """The line of `length` in nc cells, P1 or quadratic, with its dofs numbered by position: consistent mass M, lumped mass (row
    sums), stiffness S and the consistent advection matrix Adv[i][j] = int phi_i phi_j' (all CSR).  bc = "periodic": order nc dofs,
    the last cell wraps around to dof 0 -- `p1_periodic_line(nc)` at order 1 and length 1; bc = "dirichlet": order nc + 1 dofs,
    nothing prescribed -- M, lumped and S of `dirichlet_line(nc, order, length)`.  Quadratic cell e has the dofs (2e, 2e+2, 2e+1) =
    (left, right, middle); its advection matrix in that order is 1/6 [-3 -1 4; 1 3 -4; -4 4 0] (P1: 1/2 [-1 1; -1 1]); the entries
    of Adv that add up to zero (the diagonal of an inner vertex) are not stored.  The lumped mass of the periodic P1 line is stated
    as `p1_periodic_line` states it, h: the floating-point row sum 4h/6 + h/6 + h/6 is an ulp off at most sizes."""
    if order not in (1, 2) or bc not in ("periodic", "dirichlet") or nc < 2 or not length > 0.0:
        raise ValueError("order 1 or 2, bc 'periodic' or 'dirichlet', nc >= 2, length > 0")
    h = length / nc
    if order == 1:
        dofs = np.stack([np.arange(nc), np.arange(nc) + 1], axis=1)
        Me = h / 6.0 * np.array([[2.0, 1.0], [1.0, 2.0]])
        Se = 1.0 / h * np.array([[1.0, -1.0], [-1.0, 1.0]])
        Ae = 0.5 * np.array([[-1.0, 1.0], [-1.0, 1.0]])
    else:
        dofs = np.stack([2 * np.arange(nc), 2 * np.arange(nc) + 2, 2 * np.arange(nc) + 1], axis=1)
        Me = h / 30.0 * np.array([[4.0, -1.0, 2.0], [-1.0, 4.0, 2.0], [2.0, 2.0, 16.0]])
        Se = 1.0 / (3.0 * h) * np.array([[7.0, 1.0, -8.0], [1.0, 7.0, -8.0], [-8.0, -8.0, 16.0]])
        Ae = np.array([[-3.0, -1.0, 4.0], [1.0, 3.0, -4.0], [-4.0, 4.0, 0.0]]) / 6.0
    ns, nb = order * nc + (1 if bc == "dirichlet" else 0), order + 1
    dofs = dofs % ns                                     # (the periodic line's last cell ends at dof 0)
    I = np.repeat(dofs, nb, axis=1).ravel()
    J = np.tile(dofs, (1, nb)).ravel()
    M, S, Adv = (sp.coo_matrix((np.tile(E.ravel(), nc), (I, J)), shape=(ns, ns)).tocsr() for E in (Me, Se, Ae))
    Adv.eliminate_zeros()
    lumped = np.full(ns, h) if (order == 1 and bc == "periodic") else np.asarray(M.sum(axis=1)).ravel()
    return M, lumped, S, Adv


def burgers_line_ic_observed(ns: int, order: int, bc: str, ic_obs: str = "all") -> np.ndarray:
    """The dofs of slice 0 at which the initial condition is observed: "all" = every dof that is not pinned (the dirichlet line's
    dofs 0 and ns-1 are), "vertices" (order 2) = the even ones of them, a data grid with one point per cell."""
    if ic_obs not in ("all", "vertices") or (ic_obs == "vertices" and order != 2):
        raise ValueError("ic_obs 'all' or, at order 2, 'vertices'")
    obs = np.arange(ns) if bc == "periodic" else np.arange(1, ns - 1)
    return obs[obs % 2 == 0] if ic_obs == "vertices" else obs


def burgers_line_prior_from_bulk(nc: int, nt: int, dt: float, nu: float, bulk: float, ic, order: int = 2, bc: str = "periodic",
                                 length: float = 1.0, ic_noise: float = 1e8, pin: float = 1e8, ic_obs: str = "all"):
    """`burgers_prior_from_bulk` on any line of `line_operators` -- the reference's periodic quadratic line
    (scripts/burgers/solve_burgers_gmrf-fem.jl:71-72, form_prior :86-107) and the interval of _research/burgers_chen24.jl, where it is
    the construction of `burgers_chen24_batch`: returns (Q_prior, A_ic, rhs) with
        c = 1 / nu, gamma = -c bulk, tau = 0.1 sqrt(c), kappa^2 = 12 nc, Ml = diag(lumped), K = kappa^2 Ml + S, Q0 = K Ml^-1 K,
        G = Ml + dt (nu c S + gamma Adv), W = diag(1 / (dt tau^2) / lumped),
        block (t, t) = G'WG (t > 0) or Q0 (t = 0), + Ml W Ml for t < nt-1;    block (t, t-1) = -G'W Ml,
    on the dirichlet line `pin` (the reference's prescribed_noise = 1e-8) added on the diagonal of dofs 0 and ns-1 of every slice,
    A_ic the restriction to the observed dofs of slice 0 (`burgers_line_ic_observed`) and
        rhs = Q_prior(without the pins) (bulk 1) + ic_noise A_ic' ic[observed],
    ic being the whole slice (ns,).  `bulk` is meant to be mean(ic[observed]); the device prior (`BurgersLinePrior`) is tested
    against this function at its own mean.  (order 1, periodic, length 1, nu = 0.01 / pi, dt = 1 / (nt-1)) is
    `burgers_prior_from_bulk`, bit for bit."""
    M, lumped, S, Adv = line_operators(nc, order, bc, length)
    ns = lumped.shape[0]
    ic = np.asarray(ic, dtype=np.float64)
    bulk = float(bulk)
    c = 1.0 / nu
    gamma = -c * bulk
    tau = 0.1 * math.sqrt(c)
    kappa = math.sqrt(8.0 * 1.5) / math.sqrt(1.0 / nc)
    Ml = sp.diags(lumped)
    K = (kappa ** 2) * Ml + S
    Q0 = (K @ sp.diags(1.0 / lumped) @ K).tocsr()
    Gm = (Ml + dt * (nu * c * S + gamma * Adv)).tocsr()
    W = sp.diags(np.full(ns, 1.0 / (dt * tau * tau)) / lumped)
    GWG = (Gm.T @ W @ Gm).tocsr()
    MWM = (Ml.T @ W @ Ml).tocsr()
    GWM = (Gm.T @ W @ Ml).tocsr()
    pins = np.zeros(ns)
    if bc == "dirichlet":
        pins[0] = pins[-1] = pin

    def assemble(with_pins):
        blocks = [[None] * nt for _ in range(nt)]
        for t in range(nt):
            d = GWG if t > 0 else Q0
            if t < nt - 1:
                d = d + MWM
            blocks[t][t] = d + sp.diags(pins) if with_pins else d
            if t > 0:
                blocks[t][t - 1] = -GWM
                blocks[t - 1][t] = -GWM.T
        return sp.bmat(blocks, format="csr")
    free = assemble(False)
    Qp = assemble(True) if bc == "dirichlet" else free
    obs = burgers_line_ic_observed(ns, order, bc, ic_obs)
    Aic = sp.csr_matrix((np.ones(obs.size), (np.arange(obs.size), obs)), shape=(obs.size, ns * nt))
    rhs = free @ np.full(ns * nt, bulk) + ic_noise * (Aic.T @ ic[obs])
    return Qp, Aic, np.asarray(rhs)


def burgers(ns: int, nt: int, ic_noise: float = 1e8, fem_noise: float = 1e12, ic=None) -> Workload:
    """1-D viscous Burgers space-time GMRF in the time-major ordering (t-1)*ns + s:
    Q = Q_prior + ic_noise A_ic^T A_ic + fem_noise J^T J, N = nt blocks of size ns.

    Q_prior: implicit-Euler state-space blocks  G x_{t+1} = M x_t + noise  with
    G = M + dt (nu S + gamma Adv) and a Matern(alpha=2) initial precision
    (scripts/burgers/solve_burgers_gmrf-fem.jl:86-107; block structure of joint_ssm,
    SURVEY.md appendix A; stated in `burgers_prior_from_bulk`).  J = J_static + dt J_adv(u) linearised at the initial
    condition (scripts/burgers/solve_burgers_gmrf-fem.jl:118-149)."""
    nu_b = 0.01 / math.pi
    dt = 1.0 / (nt - 1)
    M, lumped, S, Adv = p1_periodic_line(ns)
    xs = np.arange(ns) / ns
    if ic is None:                                     # (another initial condition: burgers_gauss_newton_batch)
        ic = np.sin(2 * np.pi * xs) + 0.5 * np.sin(4 * np.pi * xs + 0.3)
    ic = np.asarray(ic, dtype=np.float64)
    Qp, Aic, rhs = burgers_prior_from_bulk(ns, nt, float(ic.mean()), ic, ic_noise)
    # Burgers residual tangent: rows couple slices t-1 and t only.
    u = ic
    Jadv = (sp.diags(u) @ Adv + sp.diags(Adv @ u)).tocsr()   # d/du of u u_x, lumped
    Jt = (M + dt * nu_b * S + dt * Jadv).tocsr()
    rowsJ = []
    for t in range(1, nt):
        row = [None] * nt
        row[t - 1] = -M
        row[t] = Jt
        for k in range(nt):
            if row[k] is None:
                row[k] = sp.csr_matrix((ns, ns))
        rowsJ.append(row)
    J = sp.bmat(rowsJ, format="csr")
    Q = (Qp + ic_noise * (Aic.T @ Aic) + fem_noise * (J.T @ J)).tocsc()
    Q = ((Q + Q.T) * 0.5).tocsc()
    Q.sort_indices()
    return Workload(f"burgers{ns}x{nt}", Q, rhs, nt,
                    {"dt": dt, "nu": nu_b, "nnz": int(Q.nnz)})


def burgers_gauss_newton(ns: int, nt: int, ic_noise: float = 1e8, fem_noise: float = 1e12, ic=None):
    """The pieces of the reference's Gauss-Newton loop for the Burgers space-time GMRF
    (scripts/solve_burger.jl:118-180; residual tangent scripts/burgers/solve_burgers_gmrf-fem.jl:118-149)
    on the mesh of `burgers`: returns a dict with
      Q          prior precision with the initial condition conditioned in (CSC, fixed),
      Qx_prior   Q * x_prior (information vector of the prior part),
      x_prior    starting point,
      residual   x -> r(x), the implicit-Euler Burgers residual of slices 1..nt-1 (m = ns (nt-1)),
      jacobian   x -> J(x) as CSR with ONE fixed sparsity pattern (explicit zeros kept),
      noise, n_blocks."""
    nu_b = 0.01 / math.pi
    dt = 1.0 / (nt - 1)
    M, lumped, S, Adv = p1_periodic_line(ns)
    w = burgers(ns, nt, ic_noise, 0.0, ic=ic)          # prior + initial-condition part only
    xs = np.arange(ns) / ns
    if ic is None:
        ic = np.sin(2 * np.pi * xs) + 0.5 * np.sin(4 * np.pi * xs + 0.3)
    ic = np.asarray(ic, dtype=np.float64)
    x_prior = np.full(ns * nt, float(ic.mean()))
    M = M.tocsr(); S = S.tocsr(); Adv = Adv.tocsr()
    Jstat = (M + dt * nu_b * S).tocsr()
    pat_t = (abs(Jstat) + abs(Adv) + sp.identity(ns)).tocsr()
    pat_t.data[:] = 0.0                                # explicit zeros: the union pattern of a diagonal block of J
    negM = (-M).tocsr()

    def residual(x):
        X = x.reshape(nt, ns)
        out = np.empty((nt - 1, ns))
        for t in range(1, nt):
            u = X[t]
            out[t - 1] = M @ (u - X[t - 1]) + dt * (nu_b * (S @ u) + u * (Adv @ u))
        return out.ravel()

    def jacobian(x):
        X = x.reshape(nt, ns)
        rows = []
        for t in range(1, nt):
            u = X[t]
            Jt = (Jstat + dt * (sp.diags(u) @ Adv + sp.diags(Adv @ u)) + pat_t).tocsr()
            row = [None] * nt
            row[t - 1] = negM
            row[t] = Jt
            for k in range(nt):
                if row[k] is None:
                    row[k] = sp.csr_matrix((ns, ns))
            rows.append(row)
        J = sp.bmat(rows, format="csr")
        J.sort_indices()
        return J

    return {"Q": w.Q, "Qx_prior": w.rhs, "x_prior": x_prior, "residual": residual, "jacobian": jacobian,
            "noise": fem_noise, "n_blocks": nt, "n": ns * nt, "m": ns * (nt - 1)}


def burgers_initial_conditions(ns: int, B: int, seed: int = 0) -> np.ndarray:
    """(B, ns) initial conditions a1 sin(2 pi x + p1) + a2 sin(4 pi x + p2) on the periodic line: problem 0 is the one of
    `burgers` (a1 = 1, p1 = 0, a2 = 0.5, p2 = 0.3), the others draw a1 in [0.6, 1.4], a2 in [0.2, 0.8] and both phases in
    [0, 2 pi) from `seed`."""
    rng = np.random.default_rng(seed)
    xs = np.arange(ns) / ns
    out = np.empty((B, ns))
    for p in range(B):
        a1, a2, p1, p2 = (1.0, 0.5, 0.0, 0.3) if p == 0 else (rng.uniform(0.6, 1.4), rng.uniform(0.2, 0.8),
                                                                 rng.uniform(0.0, 2 * np.pi), rng.uniform(0.0, 2 * np.pi))
        out[p] = a1 * np.sin(2 * np.pi * xs + p1) + a2 * np.sin(4 * np.pi * xs + p2)
    return out


def burgers_gauss_newton_batch(ns: int, nt: int, B: int, seed: int = 0, ic_noise: float = 1e8, fem_noise: float = 1e12):
    """A batch of Burgers Gauss-Newton problems on the mesh of `burgers_gauss_newton` -- the data-set loop of
    scripts/burgers/solve_burgers_gmrf-fem.jl:154-233, where every sample brings its own initial condition and, through
    `bulk_speed` (:86-107), its own prior.  Problem p takes `burgers_initial_conditions(ns, B, seed)[p]`; problem 0 is
    `burgers_gauss_newton(ns, nt)`.  Returns a dict with
      Q          the pattern (CSC; the values of problem 0),
      q_values   (B, nnz) values of every problem's Q on that one pattern,
      Qx_prior, x_prior   (B, n),
      x0         (B, n) start points: x_prior with the initial condition in the first slice,
      ic (B, ns), noise, n_blocks, n, m, dt, nu."""
    ics = burgers_initial_conditions(ns, B, seed)
    parts = [burgers_gauss_newton(ns, nt, ic_noise, fem_noise, ic=ics[p]) for p in range(B)]
    Q = parts[0]["Q"]
    q_values = np.empty((B, Q.nnz))
    for p, g in enumerate(parts):
        Qp = g["Q"]
        if not (np.array_equal(Qp.indptr, Q.indptr) and np.array_equal(Qp.indices, Q.indices)):
            raise ValueError(f"problem {p}: the prior's sparsity pattern differs from problem 0's")
        q_values[p] = Qp.data
    x_prior = np.stack([g["x_prior"] for g in parts])
    x0 = x_prior.copy()
    x0[:, :ns] = ics
    return {"Q": Q, "q_values": q_values, "Qx_prior": np.stack([g["Qx_prior"] for g in parts]), "x_prior": x_prior, "x0": x0,
            "ic": ics, "noise": fem_noise, "n_blocks": nt, "n": ns * nt, "m": ns * (nt - 1), "dt": 1.0 / (nt - 1),
            "nu": 0.01 / math.pi}


def dirichlet_line(nc: int, order: int = 1, length: float = 2.0):
    """The interval of `length` in nc cells, P1 or quadratic, ns = order nc + 1 dofs numbered by position: consistent mass M,
    lumped mass (row sums) and stiffness S, nothing prescribed.  Quadratic cell e has the dofs (2e, 2e+2, 2e+1) = (left, right,
    middle) with the closed-form element matrices h/30 [4 -1 2; -1 4 2; 2 2 16] and 1/(3h) [7 1 -8; 1 7 -8; -8 -8 16]."""
    h = length / nc
    if order == 1:
        dofs = np.stack([np.arange(nc), np.arange(nc) + 1], axis=1)
        Me = h / 6.0 * np.array([[2.0, 1.0], [1.0, 2.0]])
        Se = 1.0 / h * np.array([[1.0, -1.0], [-1.0, 1.0]])
    elif order == 2:
        dofs = np.stack([2 * np.arange(nc), 2 * np.arange(nc) + 2, 2 * np.arange(nc) + 1], axis=1)
        Me = h / 30.0 * np.array([[4.0, -1.0, 2.0], [-1.0, 4.0, 2.0], [2.0, 2.0, 16.0]])
        Se = 1.0 / (3.0 * h) * np.array([[7.0, 1.0, -8.0], [1.0, 7.0, -8.0], [-8.0, -8.0, 16.0]])
    else:
        raise ValueError("order 1 or 2")
    ns, nb = order * nc + 1, order + 1
    I = np.repeat(dofs, nb, axis=1).ravel()
    J = np.tile(dofs, (1, nb)).ravel()
    M = sp.coo_matrix((np.tile(Me.ravel(), nc), (I, J)), shape=(ns, ns)).tocsr()
    S = sp.coo_matrix((np.tile(Se.ravel(), nc), (I, J)), shape=(ns, ns)).tocsr()
    return M, np.asarray(M.sum(axis=1)).ravel(), S


def burgers_cole_hopf(x, t: float, nu: float, amp: float = 1.0) -> np.ndarray:
    """Burgers on the line with u(x, 0) = -amp sin(pi x) by the Cole-Hopf transform, 100-point Gauss-Hermite
    (`SolveBurgers_ColeHopf`, _research/burgers_chen24.jl:68-74, with the amplitude carried through the transform):
    u = -amp sum_k w_k sin(pi s_k) e_k / sum_k w_k e_k,  e_k = exp(-amp cos(pi s_k) / (2 pi nu)),  s_k = x - sqrt(4 nu t) z_k."""
    z, wq = np.polynomial.hermite.hermgauss(100)
    s = np.asarray(x, dtype=np.float64)[:, None] - math.sqrt(4.0 * nu * t) * z[None, :]
    e = np.exp(-amp * np.cos(np.pi * s) / (2.0 * np.pi * nu))
    return -amp * np.sum(wq * np.sin(np.pi * s) * e, axis=1) / np.sum(wq * e, axis=1)


def burgers_chen24_batch(nc: int, nt: int, B: int, nu: float, amps, order: int = 2, scheme: str = "cn", ic_noise: float = 1e12,
                         fem_noise: float = 1e12):
    """The Burgers benchmark _research/burgers_chen24.jl as a batch of Gauss-Newton problems for
    `BurgersP1Tangent(ns, nt, dt, nu, order=order, scheme=scheme, bc="dirichlet", length=2.0)`: nc cells on [-1, 1] with homogeneous
    Dirichlet ends (:101-108), ns = order nc + 1 dofs x_i = -1 + 2 i / (ns - 1), nt slices on [0, T = 1]; problem p has the initial
    condition -amps[p] sin(pi x) and the truth of `burgers_cole_hopf` at T.  Host side only.

    The prior is THIS PROJECT'S restatement, not the reference's (`form_prior`, :79-99): the package that builds that one is
    not available, and its Matern smoothness 2 / 1 (initial / spatial SPDE) is not reproduced.  It is the construction of
    `burgers_prior_from_bulk` -- implicit-Euler state-space blocks G x_{t+1} = M x_t + noise with G = M + dt (nu c S + gamma Adv),
    c = 1 / nu, gamma = -c bulk, and the Matern(alpha = 2) initial precision with range sqrt(1 / nc) -- with bulk = mean(ic) = 0
    (so the advection term drops out and every problem has the same prior), on the lumped mass and stiffness of the Dirichlet
    line's own element (`dirichlet_line`), and with the two end dofs of every slice pinned by 1e8 on their diagonal (the
    reference's prescribed_noise = 1e-8).  The initial condition is observed at the interior dofs of slice 0 with ic_noise.

    Returns the dict of `burgers_gauss_newton_batch` (Q the pattern (CSC), q_values (B, nnz), Qx_prior, x_prior, x0 (B, n), ic,
    noise, n_blocks, n, m, dt, nu; x_prior = x0 = the mean of the prior conditioned on the initial condition, Qx_prior = Q x_prior,
    as the reference passes mean(u_ic), :139-146) plus ns, nc, order, scheme, length = 2.0, amps, xs (ns,) and truth (B, ns) at T = 1."""
    if order not in (1, 2) or nc < 2 or nt < 2 or B != len(amps):
        raise ValueError("order 1 or 2, nc >= 2, nt >= 2, one amplitude per problem")
    ns = order * nc + 1
    dt = 1.0 / (nt - 1)
    xs = -1.0 + 2.0 * np.arange(ns) / (ns - 1)
    amps = np.asarray(amps, dtype=np.float64)
    ics = -amps[:, None] * np.sin(np.pi * xs)[None, :]
    ics[:, 0] = 0.0; ics[:, -1] = 0.0                   # (sin(+-pi) is 1.2e-16 in floating point)
    _, lumped, S = dirichlet_line(nc, order, 2.0)
    c = 1.0 / nu
    tau = 0.1 * math.sqrt(c)
    kappa = math.sqrt(8.0 * 1.5) / math.sqrt(1.0 / nc)
    Ml = sp.diags(lumped)
    K = (kappa ** 2) * Ml + S
    Q0 = (K @ sp.diags(1.0 / lumped) @ K).tocsr()
    Gm = (Ml + dt * (nu * c * S)).tocsr()               # (gamma = -c bulk = 0)
    W = sp.diags(np.full(ns, 1.0 / (dt * tau * tau)) / lumped)
    GWG, MWM, GWM = (Gm.T @ W @ Gm).tocsr(), (Ml.T @ W @ Ml).tocsr(), (Gm.T @ W @ Ml).tocsr()
    pin = np.zeros(ns); pin[0] = pin[-1] = 1e8
    blocks = [[None] * nt for _ in range(nt)]
    for t in range(nt):
        d = GWG if t > 0 else Q0
        if t < nt - 1:
            d = d + MWM
        blocks[t][t] = d + sp.diags(pin)
        if t > 0:
            blocks[t][t - 1] = -GWM
            blocks[t - 1][t] = -GWM.T
    Qp = sp.bmat(blocks, format="csr")
    n, m = ns * nt, ns * (nt - 1)
    interior = np.arange(1, ns - 1)
    Aic = sp.csr_matrix((np.ones(ns - 2), (np.arange(ns - 2), interior)), shape=(ns - 2, n))
    Q = (Qp + ic_noise * (Aic.T @ Aic)).tocsc()
    Q = ((Q + Q.T) * 0.5).tocsc()
    Q.sort_indices()
    # the prior conditioned on the initial condition: information vector Qp 0 + ic_noise Aic' ic, mean Q^-1 of it -- the start
    # point and the x_prior of the objective, as the reference passes mean(u_ic) for both (:139-146)
    Qx_prior = np.stack([ic_noise * (Aic.T @ ics[p, interior]) for p in range(B)])
    x_prior = np.ascontiguousarray(spla.splu(Q).solve(Qx_prior.T).T)
    x0 = x_prior.copy()
    truth = np.stack([burgers_cole_hopf(xs, 1.0, nu, float(a)) for a in amps])
    truth[:, 0] = 0.0; truth[:, -1] = 0.0
    return {"Q": Q, "q_values": np.tile(Q.data, (B, 1)), "Qx_prior": Qx_prior, "x_prior": x_prior, "x0": x0, "ic": ics,
            "noise": fem_noise, "n_blocks": nt, "n": n, "m": m, "dt": dt, "nu": nu, "ns": ns, "nc": nc, "order": order,
            "scheme": scheme, "length": 2.0, "amps": amps, "xs": xs, "truth": truth}


def burgers_collocation_points(x_coords, npts: int) -> np.ndarray:
    """The collocation grid of scripts/burgers/solve_burgers_gmrf-collocation.jl:164-165: npts points from x_coords[0] + 1/npts
    to x_coords[-1] - 1/npts, both included."""
    x_coords = np.asarray(x_coords, dtype=np.float64)
    dx = 1.0 / npts
    return np.linspace(x_coords[0] + dx, x_coords[-1] - dx, npts)


def burgers_collocation_batch(nc: int, nt: int, npts: int, B: int, nu: float, T: float, amp: float, seed: int = 0,
                              ic_noise: float = 1e8, noise: float = 1e8):
    """A batch of Gauss-Newton problems for `BurgersCollocationTangent(nc, nt, dt, nu, points)`: the data-set loop of
    scripts/burgers/solve_burgers_gmrf-collocation.jl:217-246 on nc quadratic cells of the periodic unit line (ns = 2 nc dofs
    x_i = i / ns), nt slices on [0, T], with the residual observed at `burgers_collocation_points(arange(ns) / ns, npts)` under
    `noise` (noise_collocation, :195).  Problem p has the initial condition amp * `burgers_initial_conditions(ns, B, seed)[p]`, the
    prior `burgers_line_prior_from_bulk(nc, nt, dt, nu, mean(ic), ic, order=2, bc="periodic", ic_noise=ic_noise)` with the
    initial condition observed at every dof of slice 0 (Q = Q_prior + ic_noise A_ic' A_ic), and x_ic = Q^-1 rhs, the mean of
    that conditioned prior (:224).  Host side only.

    Returns the dict of `burgers_chen24_batch`: Q the pattern (CSC; the values of problem 0), q_values (B, nnz), Qx_prior (the
    information vector of that conditioned prior, Q x_ic), x_prior = x0 = x_ic (B, n) -- the reference passes mean(x_ic) for both
    (:237, :242) --, ic (B, ns), points (npts,), noise,
    n_blocks = nt, n, m = (nt-1) npts, dt = T / (nt-1), nu, ns, nc, npts, order = 2, scheme = "collocation", length = 1.0, T, amp.

    Gauss-Newton without damping on this residual, the reference's algorithm, does not converge on coarse meshes at the
    nu = 0.01 / pi, T = 1 and amplitudes of `burgers_gauss_newton_batch`; the loop tests run at nu = 0.02, T = 0.05, amp = 0.5."""
    if nc < 3 or nt < 2 or npts < 1 or B < 1:
        raise ValueError("nc >= 3, nt >= 2, npts >= 1, B >= 1")
    ns = 2 * nc
    dt = T / (nt - 1)
    ics = amp * burgers_initial_conditions(ns, B, seed)
    points = burgers_collocation_points(np.arange(ns) / ns, npts)
    Qs, rhs = [], []
    for p in range(B):
        Qp, Aic, r = burgers_line_prior_from_bulk(nc, nt, dt, nu, float(ics[p].mean()), ics[p], order=2, bc="periodic",
                                                  ic_noise=ic_noise)
        Qc = (Qp + ic_noise * (Aic.T @ Aic)).tocsc()
        Qc = ((Qc + Qc.T) * 0.5).tocsc()
        Qc.sort_indices()
        if p and not (np.array_equal(Qc.indptr, Qs[0].indptr) and np.array_equal(Qc.indices, Qs[0].indices)):
            raise ValueError(f"problem {p}: the prior's sparsity pattern differs from problem 0's")
        Qs.append(Qc); rhs.append(r)
    x_ic = np.stack([spla.splu(Qs[p]).solve(rhs[p]) for p in range(B)])
    return {"Q": Qs[0], "q_values": np.stack([Q.data for Q in Qs]), "Qx_prior": np.stack(rhs), "x_prior": x_ic, "x0": x_ic.copy(),
            "ic": ics, "points": points, "noise": noise, "n_blocks": nt, "n": ns * nt, "m": (nt - 1) * npts, "dt": dt, "nu": nu,
            "ns": ns, "nc": nc, "npts": npts, "order": 2, "scheme": "collocation", "length": 1.0, "T": T, "amp": amp}


# --------------------------------------------------------------------------- analytic / toy

def laplace_kappa_grid(nx: int, ny: int, kappa2: float = 0.5) -> Workload:
    """5-point kappa^2 I + Delta_h on an nx x ny Dirichlet grid in row-block form:
    D_i = tridiag(-1, kappa^2+4, -1), B_i = -I, bs = nx.  Closed-form inverse via the
    discrete sine transform (SURVEY.md section 8c known-answer case (i))."""
    T = sp.diags([np.full(nx - 1, -1.0), np.full(nx, kappa2 + 4.0), np.full(nx - 1, -1.0)], [-1, 0, 1])
    E = sp.diags([np.full(ny - 1, -1.0), np.full(ny - 1, -1.0)], [-1, 1])
    Q = (sp.kron(sp.identity(ny), T) + sp.kron(E, sp.identity(nx))).tocsc()
    Q.sort_indices()
    rng = np.random.Generator(np.random.PCG64(7))
    rhs = rng.standard_normal(nx * ny)
    return Workload(f"laplace{nx}x{ny}", Q, rhs, ny, {"kappa2": kappa2, "nx": nx, "ny": ny})


def laplace_kappa_grid_variances(nx: int, ny: int, kappa2: float) -> np.ndarray:
    """Exact diag(Q^-1) of `laplace_kappa_grid` from the sine-transform eigen-decomposition."""
    i = np.arange(1, nx + 1)
    j = np.arange(1, ny + 1)
    lx = 2.0 - 2.0 * np.cos(np.pi * i / (nx + 1))
    ly = 2.0 - 2.0 * np.cos(np.pi * j / (ny + 1))
    lam = kappa2 + lx[:, None] + ly[None, :]
    sx = np.sqrt(2.0 / (nx + 1)) * np.sin(np.pi * np.outer(np.arange(1, nx + 1), i) / (nx + 1))
    sy = np.sqrt(2.0 / (ny + 1)) * np.sin(np.pi * np.outer(np.arange(1, ny + 1), j) / (ny + 1))
    var = np.einsum("xi,yj,ij->yx", sx ** 2, sy ** 2, 1.0 / lam)
    return var.ravel()


def ar1_chain_kron_identity(n_blocks: int, bs: int, phi: float = 0.5) -> Workload:
    """AR(1) chain (x) I_bs: bs independent scalar chains x_t = phi x_{t-1} + eps with a unit-variance
    start, written in block form D_1..D_{N-1} = (1 + phi^2) I except D_1 = I, D_N = I, B_i = -phi I
    (SURVEY.md section 8c known-answer case (ii)).  Closed form: L_i = I for i < N,
    L_N = sqrt(1 - phi^2) I, C_i = -phi I, logdet = bs log(1 - phi^2)."""
    d = np.full(n_blocks, 1.0 + phi * phi)
    d[0] = 1.0
    d[-1] = 1.0
    T = sp.diags([np.full(n_blocks - 1, -phi), d, np.full(n_blocks - 1, -phi)], [-1, 0, 1])
    Q = sp.kron(T, sp.identity(bs)).tocsc()
    Q.sort_indices()
    rng = np.random.Generator(np.random.PCG64(11))
    return Workload(f"ar1_{n_blocks}x{bs}", Q, rng.standard_normal(n_blocks * bs), n_blocks, {"phi": phi})


def random_block_tridiagonal(n_blocks: int, bs: int, seed: int = 0, density: float = 0.2,
                             shift: float = 2.0) -> Workload:
    """Random sparse SPD block-tridiagonal matrix (strictly block diagonally dominant)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = n_blocks * bs
    blocks = [[None] * n_blocks for _ in range(n_blocks)]
    for i in range(n_blocks):
        R = sp.random(bs, bs, density=density, random_state=rng, data_rvs=rng.standard_normal)
        blocks[i][i] = (R + R.T) * 0.5
        if i > 0:
            B = sp.random(bs, bs, density=density, random_state=rng, data_rvs=rng.standard_normal)
            blocks[i][i - 1] = B
            blocks[i - 1][i] = B.T
    A = sp.bmat(blocks, format="csr")
    rowsum = np.asarray(abs(A).sum(axis=1)).ravel()
    A = (A + sp.diags(rowsum + shift)).tocsc()
    A = ((A + A.T) * 0.5).tocsc()
    A.sort_indices()
    rhs = rng.standard_normal(n)
    return Workload(f"rand{n_blocks}x{bs}", A, rhs, n_blocks, {"seed": seed})


CONFIGS = {
    # BASELINE.json configs (SURVEY.md section 8a sizes)
    "burgers512x64": lambda: burgers(512, 64),
    "darcy64": lambda: darcy(64),
    "darcy256": lambda: darcy(256),
    "elliptic512": lambda: elliptic(512),
    "burgers4096x512": lambda: burgers(4096, 512),
    # reduced sizes for CPU-side tests
    "darcy32": lambda: darcy(32),
    "darcy16": lambda: darcy(16),
    "elliptic32": lambda: elliptic(32),
    "burgers64x8": lambda: burgers(64, 8),
}


def make(name: str) -> Workload:
    return CONFIGS[name]()


def block_bandwidth_ok(Q: sp.spmatrix, n_blocks: int) -> bool:
    """True when every stored entry lies in the block tri-band of the partition."""
    n = Q.shape[0]
    bs = n // n_blocks
    coo = Q.tocoo()
    return bool(np.all(np.abs(coo.row // bs - coo.col // bs) <= 1))
