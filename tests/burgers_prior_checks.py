"""What tests/test_burgers_prior_cpu.py and tests/test_gpu_burgers_prior.py share: the oracle of the Burgers prior built on
`workloads.burgers_prior_from_bulk`, a NumPy restatement of the stencil form the device kernels evaluate (csrc/burgers_prior.hpp),
and the tolerances of the comparison.  Not a test module."""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse as sp

EPS = float(np.finfo(np.float64).eps)
IC_NOISE = 1e8
NU = 0.01 / math.pi


def initial_conditions(W, ns, B, seed=3):
    """`workloads.burgers_initial_conditions` with a mean: the packaged ones are sums of sines, bulk = 0 to rounding, and the prior
    depends on a problem only through its bulk speed.  Problem 0 keeps its zero mean, the others get +0.7, -0.4, +1.3, -1.1, ..."""
    ics = W.burgers_initial_conditions(ns, B, seed=seed)
    shift = np.array([0.0, 0.7, -0.4, 1.3, -1.1, 0.25, -0.9, 0.55])
    return ics + shift[np.arange(B) % len(shift), None]


def oracle(W, ns, nt, bulk, ic, ic_noise=IC_NOISE):
    """(Q_ic, Q_prior, rhs) of one problem at the given bulk speed: Q_ic = Q_prior + ic_noise A_ic' A_ic, symmetrised as
    `workloads.burgers` symmetrises its Q; CSC, sorted."""
    Qp, Aic, rhs = W.burgers_prior_from_bulk(ns, nt, bulk, ic, ic_noise)
    Q = (Qp + ic_noise * (Aic.T @ Aic)).tocsc()
    Q = ((Q + Q.T) * 0.5).tocsc()
    Q.sort_indices()
    return Q, Qp.tocsr(), rhs


def stencil_coef(ns, nt, dt, nu, bulk):
    """The coefficients by |offset| as burgers_prior_coef forms them, expression by expression."""
    h = 1.0 / ns
    c = 1.0 / nu
    nuc, gamma, tau, kappa2 = nu * c, -c * bulk, 0.1 * math.sqrt(c), 12.0 * ns
    w = (1.0 / (dt * tau * tau)) / h
    g0, gp, gm = h + dt * (nuc * (2.0 / h)), dt * (nuc * (-1.0 / h) + gamma * 0.5), dt * (nuc * (-1.0 / h) + gamma * -0.5)
    k0, k1, ih, wh = kappa2 * h + 2.0 / h, -1.0 / h, 1.0 / h, w * h
    return {"d0": [(k0 * k0 + k1 * k1 + k1 * k1) * ih, (k0 * k1 + k1 * k0) * ih, (k1 * k1) * ih],
            "dg": [w * (g0 * g0 + gp * gp + gm * gm), w * (g0 * gp + gm * g0), w * (gm * gp)],
            "lo": [-(wh * g0), -(wh * gp), -(wh * gm)], "wh2": wh * h}


def stencil_matrix(pattern, ns, nt, dt, nu, ic_noise, bulk):
    """Q_ic in stencil form on `pattern` (CSC): entry by entry what burgers_prior_value returns."""
    k = stencil_coef(ns, nt, dt, nu, bulk)
    P = sp.csc_matrix(pattern)
    col = np.repeat(np.arange(P.shape[1]), np.diff(P.indptr))
    row = P.indices
    tr, ia, tc, ib = row // ns, row % ns, col // ns, col % ns
    data = np.empty(P.nnz)
    for e in range(P.nnz):
        if tr[e] == tc[e]:
            d = (ia[e] - ib[e]) % ns
            cls = 0 if d == 0 else (1 if d in (1, ns - 1) else 2)
            v = (k["d0"] if tr[e] == 0 else k["dg"])[cls]
            if cls == 0:
                if tr[e] < nt - 1:
                    v += k["wh2"]
                if tr[e] == 0:
                    v += ic_noise
        else:
            d = (ia[e] - ib[e]) % ns if tr[e] > tc[e] else (ib[e] - ia[e]) % ns
            v = k["lo"][0 if d == 0 else (1 if d == 1 else 2)]
        data[e] = v
    return sp.csc_matrix((data, P.indices, P.indptr), shape=P.shape)


def stencil_rhs(ns, nt, dt, nu, ic_noise, bulk, ic):
    """Qx_prior row by row in the order of burgers_prior_rhs_batch."""
    k = stencil_coef(ns, nt, dt, nu, bulk)
    beside = k["lo"][0] + k["lo"][1] + k["lo"][2]
    out = np.empty(ns * nt)
    for t in range(nt):
        dd = k["d0"] if t == 0 else k["dg"]
        s = 0.0
        if t > 0:
            s += beside
        s += dd[2]; s += dd[1]; s += (dd[0] + k["wh2"]) if t < nt - 1 else dd[0]; s += dd[1]; s += dd[2]
        if t < nt - 1:
            s += beside
        out[t * ns:(t + 1) * ns] = s * bulk
    out[:ns] += ic_noise * np.asarray(ic)
    return out


def value_excess(Q, Q_oracle, ns, nt):
    """max over the entries of |Q - Q_oracle| / (64 eps max|entry of that block row of the oracle|): <= 1 passes.  Every entry is a
    sum of <= 3 products of <= 3 factors on both sides, bounded by about 3 x the block's diagonal entry; 64 eps leaves about 4 x
    over that bound, a wrong stencil coefficient is wrong at O(1)."""
    A = abs(sp.csr_matrix(Q_oracle))
    row_max = A.max(axis=1).toarray().ravel()
    bound = 64.0 * EPS * np.repeat(row_max.reshape(nt, ns).max(axis=1), ns)
    D = (sp.csc_matrix(Q) - sp.csc_matrix(Q_oracle)).tocoo()
    if D.nnz == 0:
        return 0.0
    return float(np.max(np.abs(D.data) / bound[D.row]))


def rhs_excess(qx, rhs_oracle, Q_prior, ns, bulk, ic, ic_noise=IC_NOISE):
    """The same bound for Qx_prior, max|Q| replaced row by row by |Q_prior row|_1 |bulk| + ic_noise |ic| (the terms that are added)."""
    l1 = np.asarray(abs(sp.csr_matrix(Q_prior)).sum(axis=1)).ravel()
    scale = l1 * abs(bulk)
    scale[:ns] += ic_noise * np.abs(ic)
    diff = np.abs(np.asarray(qx) - rhs_oracle)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(diff == 0.0, 0.0, diff / (64.0 * EPS * scale))       # (nothing added, nothing allowed)
    return float(np.max(ratio))


def on_pattern(Q, pattern):
    """The values of Q at the stored entries of `pattern` (CSC), in its `.data` order; Q must have no entry outside it."""
    P = sp.csc_matrix(pattern)
    col = np.repeat(np.arange(P.shape[1]), np.diff(P.indptr))
    Qc = sp.csc_matrix(Q)
    vals = np.asarray(Qc[P.indices, col]).ravel()
    assert abs(sp.csc_matrix((vals, P.indices, P.indptr), shape=P.shape) - Qc).sum() == 0.0
    return vals
