"""What tests/test_burgers_line_prior_cpu.py and tests/test_gpu_burgers_line_prior.py share: the shapes, the oracle of the Burgers
line prior built on `workloads.burgers_line_prior_from_bulk`, a NumPy restatement of what the device kernels evaluate
(csrc/burgers_line_prior.hpp), expression by expression, and the bounds of the comparison.  Not a test module.

The bounds.  Device and host state the prior by the SAME expressions in the same order of summation (the rows k a product
G'WG shares ascending, an information-vector row's columns ascending); they differ in three inputs and in what follows from them:
  * the lumped mass l: the host sums a row of the assembled mass matrix, the device adds the cells' row sums; each is at most 3
    roundings from the exact value (two products and an addition inside a cell, one addition across cells): 6 eps between them;
  * kappa^2: the host squares sqrt(12) / sqrt(1 / nc) (two roots, two divisions, a product: 5 roundings), the device writes 12 nc
    (exact): 5 eps;
  * the device compiler may contract a product and the sum it feeds into one rounding.
An entry is sum_k (X_ka w_k) X_kb over at most 2 order + 1 <= 5 rows, X = G or K, w_k = wnum / l_k.  l enters X_ka, X_kb (their
diagonal term) and w_k: 3 x 6 = 18 eps, kappa^2 enters K twice: 10 eps, and of the operations downstream of those inputs -- one
addition inside each X, the division of w_k, two products, four additions of the sum, the three operations of l w l and its
addition -- each can round differently on the two sides or be contracted away: 12 eps.  That is 40 eps times sum_k |X_ka| w_k |X_kb|,
which Cauchy-Schwarz bounds by sqrt(D_aa D_bb) <= the block row's largest entry (D the block's diagonal): VALUE_K = 64 leaves 1.6 x.
An information-vector row adds at most (2 order + 1) + (4 order + 1) + (2 order + 1) = 19 entries.  18 additions on either side,
each within eps of a partial sum <= |row|_1 |bulk|: 36; the host multiplies every entry by bulk, the device the sum: 2; ic_noise ic
is a product and an addition on either side: 4 -- 42 for the summation.  The entries themselves differ by the 40 eps above, not of
|Q_rc| but of sum_k |X_kr| w_k |X_kc|; the stiffness rows (1, -8, 14, -8, 1) / (3h) and (-8, 16, -8) / (3h) make terms of both
signs, and summed over a row the absolute terms stand at most about 2 x over |row|_1: 80.  42 + 80 = 122: RHS_K = 128.
(The P1 stencil prior's 64 covers 11 entries of coefficients formed once; it is not reused here.)"""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse as sp

from tests import burgers_prior_checks as BP

EPS = BP.EPS
NU = BP.NU
VALUE_K = 64.0
RHS_K = 128.0

# (order, bc, nc, nt): the smallest at which each mechanism can go wrong
SHAPES = [(2, "periodic", 5, 2), (2, "periodic", 20, 5), (2, "periodic", 32, 8),
          (2, "dirichlet", 4, 3), (2, "dirichlet", 32, 6),
          (1, "dirichlet", 2, 2), (1, "dirichlet", 40, 5),
          (1, "periodic", 64, 8), (1, "periodic", 5, 2)]
VERTEX_SHAPES = [(2, "periodic", 20, 5), (2, "dirichlet", 32, 6)]
CASES = [s + ("all",) for s in SHAPES] + [s + ("vertices",) for s in VERTEX_SHAPES]


class Cfg:
    """One line prior: what gmrf_burgers_line_prior_create takes, and what BurgersLinePriorArgs holds."""

    def __init__(self, order, bc, nc, nt, ic_obs="all", nu=NU, ic_noise=1e8, pin=1e8, length=None, dt=None):
        self.order, self.bc, self.nc, self.nt, self.ic_obs, self.nu, self.ic_noise = order, bc, nc, nt, ic_obs, nu, ic_noise
        self.periodic = bc == "periodic"
        self.length = (1.0 if self.periodic else 2.0) if length is None else length
        self.pin = 0.0 if self.periodic else pin
        self.dt = 1.0 / (nt - 1) if dt is None else dt
        self.ns = order * nc + (0 if self.periodic else 1)
        self.n = self.ns * nt
        self.h = self.length / nc
        self.vertices = ic_obs == "vertices"

    def prior(self, pkg, device=-1, stream=0):
        return pkg.BurgersLinePrior(self.nc, self.nt, self.dt, self.nu, order=self.order, bc=self.bc, length=self.length,
                                    ic_noise=self.ic_noise, pin=self.pin if not self.periodic else 1e8, ic_obs=self.ic_obs,
                                    device=device, stream=stream)

    def observed(self, W):
        return W.burgers_line_ic_observed(self.ns, self.order, self.bc, self.ic_obs)

    def nnz(self):
        o, ns, nt = self.order, self.ns, self.nt
        if self.periodic:
            return ((4 * o + 1) * nt + 2 * (2 * o + 1) * (nt - 1)) * ns
        return nt * ((4 * o + 1) * ns - 2 * o * (2 * o + 1)) + 2 * (nt - 1) * ((2 * o + 1) * ns - o * (o + 1))

    def __repr__(self):
        return f"P{self.order} {self.bc} {self.nc}x{self.nt} {self.ic_obs}"


def initial_conditions(W, cfg, B):
    """`burgers_prior_checks.initial_conditions` (non-zero bulks) on the line's dofs; zero at the ends of a dirichlet line."""
    ics = BP.initial_conditions(W, cfg.ns, B)
    if not cfg.periodic:
        ics[:, 0] = 0.0
        ics[:, -1] = 0.0
    return ics


def oracle(W, cfg, bulk, ic):
    """(Q_ic, Q_prior without the pins (CSR), rhs) of one problem at the given bulk speed: Q_ic = Q_prior + ic_noise A_ic' A_ic,
    symmetrised as `workloads.burgers` symmetrises its Q; CSC, sorted."""
    Qp, Aic, rhs = W.burgers_line_prior_from_bulk(cfg.nc, cfg.nt, cfg.dt, cfg.nu, bulk, ic, cfg.order, cfg.bc, cfg.length, cfg.ic_noise,
                                                  cfg.pin, cfg.ic_obs)
    Q = (Qp + cfg.ic_noise * (Aic.T @ Aic)).tocsc()
    Q = ((Q + Q.T) * 0.5).tocsc()
    Q.sort_indices()
    pins = np.zeros(cfg.n)
    if not cfg.periodic:
        pins[0::cfg.ns] = cfg.pin
        pins[cfg.ns - 1::cfg.ns] = cfg.pin
    return Q, (Qp - sp.diags(pins)).tocsr(), rhs


# ------------------------------------------------------------------------------------------------ the kernels' arithmetic in NumPy
_S1, _A1 = [[1.0, -1.0], [-1.0, 1.0]], [[-1.0, 1.0], [-1.0, 1.0]]
_S2 = [[7.0, 1.0, -8.0], [1.0, 7.0, -8.0], [-8.0, -8.0, 16.0]]
_A2 = [[-3.0, -1.0, 4.0], [1.0, 3.0, -4.0], [-4.0, 4.0, 0.0]]


def _local(order, u):
    return u if order == 1 else (0 if u == 0 else (1 if u == 2 else 2))


def _cells(cfg, i):
    if cfg.order == 1:
        first, count = i - 1, 2
    elif i & 1:
        first, count = (i - 1) // 2, 1
    else:
        first, count = i // 2 - 1, 2
    return [e for e in range(first, first + count) if cfg.periodic or 0 <= e < cfg.nc]


def _mass_rowsum(cfg, li):
    h = cfg.h
    if cfg.order == 1:
        return h / 6.0 * 2.0 + h / 6.0 * 1.0
    m = h / 30.0
    return m * 2.0 + m * 2.0 + m * 16.0 if li == 2 else (m * 4.0 + m * -1.0 + m * 2.0 if li == 0 else m * -1.0 + m * 4.0 + m * 2.0)


def _lumped(cfg, i):
    l = 0.0
    for e in _cells(cfg, i):
        l += _mass_rowsum(cfg, _local(cfg.order, i - cfg.order * e))
    return l


def _sa(cfg, i, d):
    s = adv = 0.0
    for e in _cells(cfg, i):
        ui = i - cfg.order * e
        uj = ui + d
        if uj < 0 or uj > cfg.order:
            continue
        li, lj = _local(cfg.order, ui), _local(cfg.order, uj)
        if cfg.order == 1:
            s += 1.0 / cfg.h * _S1[li][lj]
            adv += 0.5 * _A1[li][lj]
        else:
            s += 1.0 / (3.0 * cfg.h) * _S2[li][lj]
            adv += _A2[li][lj] / 6.0
    return s, adv


def coef(cfg, bulk, gamma_sign=1.0):
    """burgers_line_prior_coef; gamma_sign = -1 is the wrong sign of the advection term."""
    c = 1.0 / cfg.nu
    tau = 0.1 * math.sqrt(c)
    return {"nuc": cfg.nu * c, "gamma": gamma_sign * (-c * bulk), "kappa2": 12.0 * float(cfg.nc), "wnum": 1.0 / (cfg.dt * tau * tau)}


def _G(cfg, q, k, d, lk):
    s, adv = _sa(cfg, k, d)
    g = cfg.dt * (q["nuc"] * s + q["gamma"] * adv)
    return lk + g if d == 0 else g


def _K(cfg, q, k, d, lk):
    s, _ = _sa(cfg, k, d)
    return q["kappa2"] * lk + s if d == 0 else s


def _dist(cfg, k, j):
    d = j - k
    if cfg.periodic:
        if 2 * d > cfg.ns:
            d -= cfg.ns
        elif 2 * d < -cfg.ns:
            d += cfg.ns
    return d


def _observed(cfg, i):
    if not cfg.periodic and i in (0, cfg.ns - 1):
        return False
    return not (cfg.vertices and (i & 1))


def _ascending(cfg, centre, R):
    """(offset, index) of centre - R .. centre + R in ascending index: wrapped from beyond ns-1, in range, wrapped from below 0."""
    out = []
    for where in range(3):
        for o in range(-R, R + 1):
            k = centre + o
            w = 0 if k >= cfg.ns else (1 if k >= 0 else 2)
            if w != where:
                continue
            if w != 1:
                if not cfg.periodic:
                    continue
                k += -cfg.ns if w == 0 else cfg.ns
            out.append((o, k))
    return out


def value(cfg, q, row, col, closed=True):
    """burgers_line_prior_value."""
    ns, R = cfg.ns, cfg.order
    tr, ia, tc, ib = row // ns, row % ns, col // ns, col % ns
    if tr != tc:
        b, later = (ib, ia) if tr > tc else (ia, ib)
        lb = _lumped(cfg, b)
        return -((_G(cfg, q, b, _dist(cfg, b, later), lb) * (q["wnum"] / lb)) * lb)
    lo, hi = min(ia, ib), max(ia, ib)
    v = 0.0
    for o, k in _ascending(cfg, lo, R):
        dh = _dist(cfg, k, hi)
        if dh < -R or dh > R:
            continue
        lk = _lumped(cfg, k)
        if tr == 0:
            v += (_K(cfg, q, k, -o, lk) * (1.0 / lk)) * _K(cfg, q, k, dh, lk)
        else:
            v += (_G(cfg, q, k, -o, lk) * (q["wnum"] / lk)) * _G(cfg, q, k, dh, lk)
    if ia == ib:
        if tr < cfg.nt - 1:
            l = _lumped(cfg, ia)
            v += (l * (q["wnum"] / l)) * l
        if closed:
            if not cfg.periodic and ia in (0, ns - 1):
                v += cfg.pin
            if tr == 0 and _observed(cfg, ia):
                v += cfg.ic_noise
    return v


def restated_matrix(pattern, cfg, bulk, gamma_sign=1.0):
    """Q_ic on `pattern` (CSC): entry by entry what burgers_line_prior_values_batch stores."""
    q = coef(cfg, bulk, gamma_sign)
    P = sp.csc_matrix(pattern)
    col = np.repeat(np.arange(P.shape[1]), np.diff(P.indptr))
    data = np.array([value(cfg, q, int(r), int(c)) for r, c in zip(P.indices, col)])
    return sp.csc_matrix((data, P.indices, P.indptr), shape=P.shape)


def restated_rhs(cfg, bulk, ic):
    """Qx_prior row by row in the order of burgers_line_prior_rhs_batch."""
    q = coef(cfg, bulk)
    ns, out = cfg.ns, np.empty(cfg.n)
    for r in range(cfg.n):
        t, i = r // ns, r % ns
        s = 0.0
        for tc in (t - 1, t, t + 1):
            if tc < 0 or tc >= cfg.nt:
                continue
            for _, c in _ascending(cfg, i, 2 * cfg.order if tc == t else cfg.order):
                s += value(cfg, q, r, tc * ns + c, closed=False)
        v = s * bulk
        if t == 0 and _observed(cfg, i):
            v += cfg.ic_noise * ic[i]
        out[r] = v
    return out


def restated_bulk(cfg, ic):
    """burgers_line_bulk_batch: thread t adds its observed dofs among t, t + 256, ..., then the tree over 256 partial sums."""
    red = np.zeros(256)
    for i in range(cfg.ns):
        if _observed(cfg, i):
            red[i % 256] += ic[i]
    w = 128
    while w > 0:
        red[:w] = red[:w] + red[w:2 * w]
        w >>= 1
    count = sum(1 for i in range(cfg.ns) if _observed(cfg, i))
    return red[0] / float(count)


# ------------------------------------------------------------------------------------------------ the bounds
def value_excess(Q, Q_oracle, cfg):
    """max over the entries of |Q - Q_oracle| / (VALUE_K eps max|entry of that block row of the oracle|): <= 1 passes."""
    A = abs(sp.csr_matrix(Q_oracle))
    row_max = A.max(axis=1).toarray().ravel()
    bound = VALUE_K * EPS * np.repeat(row_max.reshape(cfg.nt, cfg.ns).max(axis=1), cfg.ns)
    D = (sp.csc_matrix(Q) - sp.csc_matrix(Q_oracle)).tocoo()
    if D.nnz == 0:
        return 0.0
    return float(np.max(np.abs(D.data) / bound[D.row]))


def rhs_excess(qx, rhs_oracle, Q_prior, cfg, bulk, ic, W):
    """max over the rows of |qx - rhs| / (RHS_K eps (|Q_prior row|_1 |bulk| + ic_noise |ic at an observed dof|))."""
    l1 = np.asarray(abs(sp.csr_matrix(Q_prior)).sum(axis=1)).ravel()
    scale = l1 * abs(bulk)
    obs = cfg.observed(W)
    scale[obs] += cfg.ic_noise * np.abs(np.asarray(ic)[obs])
    diff = np.abs(np.asarray(qx) - rhs_oracle)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(diff == 0.0, 0.0, diff / (RHS_K * EPS * scale))       # (nothing added, nothing allowed)
    return float(np.max(ratio))


def bulk_tol(cfg, ic):
    return 2 * np.log2(cfg.ns) * EPS * float(np.mean(np.abs(np.asarray(ic))))
