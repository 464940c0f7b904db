"""SciPy restatement of the Burgers collocation tangent -- gmrf_burgers_colloc_create -- and of the batched Gauss-Newton loop
on it, on SuperLU.  Written as scripts/burgers/solve_burgers_gmrf-collocation.jl writes it: the three point operators of
:167-169 on the periodic quadratic line, their space-time forms (:172-175, `vcat` of `spatial_to_spatiotemporal` blocks),
`J_static` (:183) and `f_and_J` (:186-192).  Not a test module.

Mesh: nc cells of length h = length / nc, ns = 2 nc dofs numbered by position, cell e with the dofs (left, right, middle) =
(2e, (2e+2) mod ns, 2e+1).  A point x lies in the cell e = min(floor(x / h), nc - 1) at xi = 2 (x - e h) / h - 1, with
    shape values        (xi (xi - 1) / 2, xi (xi + 1) / 2, 1 - xi^2)
    first derivatives   (xi - 1/2, xi + 1/2, -2 xi) 2 / h
    second derivatives  (1, 1, -2) 4 / h^2."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from tests import gn_batch_oracle as GO
from tests.burgers_cn_oracle import batch_loop, gn_step, logdet, posterior_matrix      # noqa: F401  (reused as they are)
from tests.gn_batch_oracle import problem_matrix, stop_margin                           # noqa: F401


def special_points(nc, npts, length=1.0, seed=0):
    """npts >= 7 points in [0, length), shuffled: 0.0, an inner vertex, a midpoint, two points in one cell, one in the wrap cell,
    the rest uniform."""
    h = length / nc
    fixed = [0.0, 2 * h, 2.5 * h, 1.15 * h, 1.35 * h, (nc - 1 + 0.65) * h]
    rng = np.random.default_rng(seed)
    pts = np.concatenate([fixed, rng.uniform(0.0, length, npts - len(fixed))])
    assert pts.size == npts and np.all(pts >= 0.0) and np.all(pts < length)
    return rng.permutation(pts)


def colloc_operators(nc: int, points, length: float = 1.0):
    """(A, D1, D2): CSR, npts x ns, three stored entries per row (zeros kept), sorted indices -- evaluation_matrix,
    derivative_matrices and second_derivative_matrices of the script at `points`."""
    x = np.asarray(points, dtype=np.float64)
    ns, h = 2 * nc, length / nc
    e = np.minimum(np.floor(x / h), nc - 1)
    xi = 2.0 * (x - e * h) / h - 1.0
    e = e.astype(np.int64)
    cols = np.stack([2 * e, (2 * e + 2) % ns, 2 * e + 1], axis=1)
    a = np.stack([0.5 * xi * (xi - 1.0), 0.5 * xi * (xi + 1.0), 1.0 - xi * xi], axis=1)
    d = np.stack([(xi - 0.5) * (2.0 / h), (xi + 0.5) * (2.0 / h), (-2.0 * xi) * (2.0 / h)], axis=1)
    s = np.tile(np.array([1.0, 1.0, -2.0]) * (4.0 / (h * h)), (x.size, 1))
    rows = np.repeat(np.arange(x.size), 3)
    out = []
    for v in (a, d, s):
        M = sp.coo_matrix((v.ravel(), (rows, cols.ravel())), shape=(x.size, ns)).tocsr()
        M.sort_indices()
        assert M.nnz == 3 * x.size
        out.append(M)
    return tuple(out)


def spatial_to_spatiotemporal(E, t: int, nt: int):
    """E (npts x ns) acting on slice t (0-based) of the time-major space-time vector: npts x nt ns."""
    return sp.hstack([E if k == t else sp.csr_matrix(E.shape) for k in range(nt)], format="csr")


def _with_zeros(J, P):
    """J (sorted CSR, zeros possibly pruned by SciPy's arithmetic) on the pattern P (sorted CSR), explicit zeros restored."""
    J = sp.csr_matrix(J); J.sort_indices()
    key = lambda M: np.repeat(np.arange(M.shape[0], dtype=np.int64), np.diff(M.indptr)) * M.shape[1] + M.indices
    kP, kJ = key(P), key(J)
    pos = np.searchsorted(kP, kJ)
    assert np.array_equal(kP[pos], kJ)
    data = np.zeros(P.nnz)
    data[pos] = J.data
    return sp.csr_matrix((data, P.indices.copy(), P.indptr.copy()), shape=P.shape)


def f_and_J(nc, nt, dt, nu, points, w, length=1.0):
    """(f, J) of the script: J as CSR ((nt-1) npts x nt ns), sorted indices, explicit zeros kept -- row (t-1) npts + c holds the
    three dofs of point c's cell in slice t-1, then in slice t."""
    A, D1, D2 = colloc_operators(nc, points, length)
    w = np.asarray(w, dtype=np.float64)
    vc = lambda E, ts: sp.vstack([spatial_to_spatiotemporal(E, t, nt) for t in ts], format="csr")
    At, At1 = vc(A, range(nt - 1)), vc(A, range(1, nt))
    D1t1, D2t1 = vc(D1, range(1, nt)), vc(D2, range(1, nt))
    J_static = At1 - At - dt * nu * D2t1
    At1_w, D1t1_w = At1 @ w, D1t1 @ w
    f = At1_w - At @ w + dt * At1_w * D1t1_w - dt * nu * (D2t1 @ w)
    J = J_static + dt * (sp.diags(D1t1_w) @ At1 + sp.diags(At1_w) @ D1t1)
    ones = sp.csr_matrix((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape)
    P = (vc(ones, range(nt - 1)) + vc(ones, range(1, nt))).tocsr()
    P.sort_indices()
    return np.asarray(f), _with_zeros(J, P)


# The case of the loop tests (tests/test_burgers_colloc_cpu.py on the oracle alone, tests/test_gpu_burgers_colloc.py on the
# device).  A mild regime: at the nu = 0.01 / pi, T = 1 and amplitudes ~ 1 of the FEM loop's tests the undamped loop does not stop
# on 16 to 32 cells.
COLLOC_CASE = {"nc": 20, "nt": 6, "npts": 27, "B": 6, "seed": 0, "nu": 0.02, "T": 0.05, "amp": 0.5, "ic_noise": 1e8, "noise": 1e8,
               "rtol": 3e-5, "max_steps": 12}


def colloc_case(workloads, **over):
    """(workload, fJ, Qs, batch_loop result) of COLLOC_CASE."""
    c = dict(COLLOC_CASE, **over)
    w = workloads.burgers_collocation_batch(c["nc"], c["nt"], c["npts"], c["B"], c["nu"], c["T"], c["amp"], seed=c["seed"],
                                            ic_noise=c["ic_noise"], noise=c["noise"])

    def fJ(x):
        return f_and_J(c["nc"], c["nt"], w["dt"], w["nu"], w["points"], x, w["length"])

    Qs = [GO.problem_matrix(w["Q"], w["q_values"][p]) for p in range(c["B"])]
    return w, fJ, Qs, batch_loop(fJ, Qs, w["Qx_prior"], w["x_prior"], w["x0"], w["noise"], c["rtol"], c["max_steps"])
