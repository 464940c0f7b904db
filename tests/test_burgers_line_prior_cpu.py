"""The Burgers line prior without a GPU: the host statement (`workloads.line_operators`, `burgers_line_prior_from_bulk`) against
the functions it generalises, the structural pattern of `BurgersLinePrior` (device = -1) with its refusals, and -- on the CPU, in
NumPy -- that the arithmetic of csrc/burgers_line_prior.hpp meets the bounds tests/test_gpu_burgers_line_prior.py holds the device to."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

from tests import burgers_line_prior_checks as LP
from tests import burgers_prior_checks as BP

SMALLEST = [(2, "periodic", 5, 2), (2, "dirichlet", 4, 3), (1, "dirichlet", 2, 2), (1, "periodic", 5, 2)]


def _same(a, b):
    return (sp.csr_matrix(a) != sp.csr_matrix(b)).nnz == 0


# ------------------------------------------------------------------------------------------------ host statement
@pytest.mark.parametrize("ns", [64, 5])
def test_line_operators_are_the_p1_periodic_line(pkg, ns):
    W = pkg.workloads
    M, lumped, S, Adv = W.p1_periodic_line(ns)
    M2, lumped2, S2, Adv2 = W.line_operators(ns, 1, "periodic", 1.0)
    assert _same(M, M2) and _same(S, S2) and _same(Adv, Adv2) and np.array_equal(lumped, lumped2)


@pytest.mark.parametrize("nc,order", [(8, 1), (8, 2), (2, 1), (4, 2)])
def test_line_operators_are_the_dirichlet_line(pkg, nc, order):
    W = pkg.workloads
    M, lumped, S = W.dirichlet_line(nc, order, 2.0)
    M2, lumped2, S2, _ = W.line_operators(nc, order, "dirichlet", 2.0)
    assert _same(M, M2) and _same(S, S2) and np.array_equal(lumped, lumped2)


@pytest.mark.parametrize("order,bc", [(1, "periodic"), (2, "periodic"), (1, "dirichlet"), (2, "dirichlet")])
def test_advection_matrix_by_quadrature(pkg, order, bc):
    """Adv[i][j] = int phi_i phi_j' with the Lagrange basis written out here and a 4-point Gauss rule (exact to degree 7; the
    integrand has degree 2 order - 1), cell by cell; and the quadratic element's matrix in (left, right, middle) order."""
    nc, length = 6, 1.7
    h = length / nc
    xg, wg = np.polynomial.legendre.leggauss(4)
    xi = 0.5 * (xg + 1.0)                                   # reference cell [0, 1]
    if order == 1:
        phi = np.stack([1 - xi, xi])
        dphi = np.stack([-np.ones_like(xi), np.ones_like(xi)])
        local = lambda e: [e, e + 1]
    else:                                                   # (left, right, middle)
        phi = np.stack([(1 - xi) * (1 - 2 * xi), xi * (2 * xi - 1), 4 * xi * (1 - xi)])
        dphi = np.stack([4 * xi - 3, 4 * xi - 1, 4 - 8 * xi])
        local = lambda e: [2 * e, 2 * e + 2, 2 * e + 1]
    Ae = np.einsum("iq,jq,q->ij", phi, dphi / h, 0.5 * wg * h)
    if order == 2:
        assert np.max(np.abs(Ae - np.array([[-3, -1, 4], [1, 3, -4], [-4, 4, 0]]) / 6.0)) < 8 * BP.EPS
    ns = order * nc + (1 if bc == "dirichlet" else 0)
    A = np.zeros((ns, ns))
    for e in range(nc):
        d = np.array(local(e)) % ns
        A[np.ix_(d, d)] += Ae
    Adv = pkg.workloads.line_operators(nc, order, bc, length)[3].toarray()
    assert np.max(np.abs(Adv - A)) < 8 * BP.EPS
    assert np.max(np.abs(Adv @ np.ones(ns))) < 8 * BP.EPS        # the derivative of a constant


@pytest.mark.parametrize("ns,nt", [(64, 8), (5, 2)])
@pytest.mark.parametrize("bulk", [0.0, 0.7])
def test_the_p1_periodic_line_gives_burgers_prior_from_bulk(pkg, ns, nt, bulk):
    W = pkg.workloads
    ic = W.burgers_initial_conditions(ns, 2)[1] + bulk
    Qp, _, rhs = W.burgers_prior_from_bulk(ns, nt, bulk, ic, 1e8)
    Qp2, Aic2, rhs2 = W.burgers_line_prior_from_bulk(ns, nt, 1.0 / (nt - 1), 0.01 / math.pi, bulk, ic, 1, "periodic", 1.0, 1e8)
    assert (Qp != Qp2).nnz == 0 and np.array_equal(rhs, rhs2)
    assert Aic2.shape == (ns, ns * nt) and (Aic2 != sp.identity(ns * nt, format="csr")[:ns]).nnz == 0


@pytest.mark.parametrize("order", [1, 2])
def test_the_dirichlet_line_gives_burgers_chen24_batch(pkg, order):
    W = pkg.workloads
    w = W.burgers_chen24_batch(8, 4, 2, 0.02, (1.0, 0.5), order=order)
    for p in range(2):
        cfg = LP.Cfg(order, "dirichlet", 8, 4, nu=0.02, ic_noise=1e12)
        Q, _, rhs = LP.oracle(W, cfg, 0.0, w["ic"][p])
        assert (Q != w["Q"]).nnz == 0 and np.array_equal(rhs, w["Qx_prior"][p])


@pytest.mark.parametrize("order,bc,nc,nt", SMALLEST)
def test_prior_is_symmetric_positive_definite(pkg, order, bc, nc, nt):
    cfg = LP.Cfg(order, bc, nc, nt)
    for bulk in (0.0, 0.7, -1.1):
        Qp = pkg.workloads.burgers_line_prior_from_bulk(nc, nt, cfg.dt, cfg.nu, bulk, np.zeros(cfg.ns), order, bc, cfg.length)[0].toarray()
        scale = np.max(np.abs(Qp))
        assert np.max(np.abs(Qp - Qp.T)) <= 8 * BP.EPS * scale
        ev = np.linalg.eigvalsh(0.5 * (Qp + Qp.T))
        print(f"{cfg} bulk {bulk}: eigenvalues in [{ev[0]:.3e}, {ev[-1]:.3e}]")
        assert ev[0] > cfg.n * BP.EPS * ev[-1]


# ------------------------------------------------------------------------------------------------ pattern
@pytest.mark.parametrize("order,bc,nc,nt,ic_obs", LP.CASES)
def test_pattern_is_symmetric_sorted_and_block_tridiagonal(pkg, order, bc, nc, nt, ic_obs):
    cfg = LP.Cfg(order, bc, nc, nt, ic_obs)
    prior = cfg.prior(pkg)
    P, ns, n = prior.pattern, cfg.ns, cfg.n
    assert (prior.ns, prior.n, prior.nnz) == (ns, n, cfg.nnz()) and P.shape == (n, n) and P.nnz == cfg.nnz()
    assert all(np.all(np.diff(P.indices[P.indptr[j]:P.indptr[j + 1]]) > 0) for j in range(n))        # ascending, no duplicates
    assert abs(P - P.T).nnz == 0
    assert pkg.workloads.block_bandwidth_ok(P, nt)
    # the offsets per block: exactly 0 .. +-2 order in the diagonal blocks and 0 .. +-order beside them, every one of them at every
    # column it is in range of (dirichlet) or wrapped (periodic)
    got = set(zip(*P.nonzero()))
    want = set()
    for t in range(nt):
        for tb, R in ((t - 1, order), (t, 2 * order), (t + 1, order)):
            if 0 <= tb < nt:
                for i in range(ns):
                    for o in range(-R, R + 1):
                        j = i + o
                        if cfg.periodic or 0 <= j < ns:
                            want.add((tb * ns + j % ns, t * ns + i))
    assert got == want


@pytest.mark.parametrize("order,bc,nc,nt,ic_obs", LP.CASES)
def test_pattern_contains_the_host_statements_pattern(pkg, order, bc, nc, nt, ic_obs):
    cfg = LP.Cfg(order, bc, nc, nt, ic_obs)
    P = cfg.prior(pkg).pattern
    ic = LP.initial_conditions(pkg.workloads, cfg, 2)[1]
    Q = LP.oracle(pkg.workloads, cfg, 0.7, ic)[0].copy()
    Q.eliminate_zeros()
    Q.data[:] = 1.0
    assert (Q - Q.multiply(P)).nnz == 0 and abs(Q - Q.multiply(P)).sum() == 0.0
    print(f"{cfg}: host nnz {Q.nnz}, structural nnz {P.nnz}")


def test_p1_periodic_pattern_is_the_p1_priors(pkg):
    for ns, nt in ((64, 8), (5, 2)):
        a = pkg.BurgersP1Prior(ns, nt, 1.0 / (nt - 1), LP.NU, device=-1).pattern
        b = LP.Cfg(1, "periodic", ns, nt).prior(pkg).pattern
        assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)


@pytest.mark.parametrize("kwargs,named", [
    (dict(order=3), "order"), (dict(bc=7), "bc"), (dict(ic_obs=5), "ic_obs"), (dict(order=1, ic_obs=1), "vertices"),
    (dict(length=0.0), "length"), (dict(nu=0.0), "nu"), (dict(dt=0.0), "dt"), (dict(pin=-1.0), "pin"), (dict(nt=1), "nt"),
    (dict(order=2, bc=0, nc=4), "order * nc"), (dict(order=1, bc=0, nc=4), "order * nc"), (dict(bc=1, nc=1), "nc")])
def test_refusals_name_the_argument(pkg, lib, kwargs, named):
    import ctypes as C
    a = dict(nc=8, nt=4, dt=0.25, nu=LP.NU, ic_noise=1e8, order=2, bc=0, length=1.0, pin=1e8, ic_obs=0)
    a.update(kwargs)
    h = C.c_void_p()
    st = lib.gmrf_burgers_line_prior_create(-1, None, a["nc"], a["nt"], a["dt"], a["nu"], a["ic_noise"], a["order"], a["bc"], a["length"],
                                            a["pin"], a["ic_obs"], C.byref(h))
    assert st == pkg._cabi.ERR_BAD_SHAPE and not h.value
    with pytest.raises(pkg.GmrfError) as e:
        pkg._cabi.check(st)
    print(e.value)
    assert named in str(e.value)


def test_the_smallest_lines_are_accepted_and_values_need_the_device(pkg):
    assert LP.Cfg(2, "periodic", 5, 2).prior(pkg).ns == 10 and LP.Cfg(1, "periodic", 5, 2).prior(pkg).ns == 5
    assert LP.Cfg(2, "dirichlet", 2, 2).prior(pkg).ns == 5 and LP.Cfg(1, "dirichlet", 2, 2).prior(pkg).ns == 3
    for bad in (dict(bc="open"), dict(ic_obs="middles")):
        with pytest.raises(pkg.GmrfError) as e:
            pkg.BurgersLinePrior(8, 4, 0.25, LP.NU, device=-1, **bad)
        assert e.value.status == pkg._cabi.ERR_BAD_SHAPE
    with pytest.raises(pkg.GmrfError) as e:        # the numeric phase needs the GPU: no CPU fallback
        LP.Cfg(2, "periodic", 8, 3).prior(pkg).values_batch(np.zeros((2, 16)))
    assert e.value.status == pkg._cabi.ERR_NO_DEVICE


# ------------------------------------------------------------------------------------------------ the kernels' arithmetic
@pytest.mark.parametrize("order,bc,nc,nt,ic_obs", LP.CASES)
def test_restated_kernels_meet_the_bounds(pkg, order, bc, nc, nt, ic_obs):
    """The arithmetic of csrc/burgers_line_prior.hpp, written in NumPy, against the host statement within the bounds the device is
    held to -- and at or below half of them: the restatement has no contraction and shares the host's arithmetic."""
    W, B = pkg.workloads, 3
    cfg = LP.Cfg(order, bc, nc, nt, ic_obs)
    P = cfg.prior(pkg).pattern
    ics = LP.initial_conditions(W, cfg, B)
    for p in range(B):
        obs = cfg.observed(W)
        bulk = LP.restated_bulk(cfg, ics[p])
        assert abs(bulk - ics[p][obs].mean()) <= LP.bulk_tol(cfg, ics[p])
        Q, Qfree, rhs = LP.oracle(W, cfg, bulk, ics[p])
        R = LP.restated_matrix(P, cfg, bulk)
        assert abs(R - R.T).nnz == 0                                  # bitwise symmetric
        ev = LP.value_excess(R, Q, cfg)
        er = LP.rhs_excess(LP.restated_rhs(cfg, bulk, ics[p]), rhs, Qfree, cfg, bulk, ics[p], W)
        print(f"{cfg} p={p} bulk {bulk:+.3f}: values at {ev:.4f} of the {LP.VALUE_K:.0f}-eps bound, Qx_prior at {er:.4f} of the {LP.RHS_K:.0f}-eps bound")
        assert ev <= 0.5 and er <= 0.5
    # a wrong coefficient is far outside: the sign of the advection term (problem 1's bulk speed is not zero)
    bulk = LP.restated_bulk(cfg, ics[1])
    assert abs(bulk) > 0.1
    bad = LP.restated_matrix(P, cfg, bulk, gamma_sign=-1.0)
    assert LP.value_excess(bad, LP.oracle(W, cfg, bulk, ics[1])[0], cfg) > 1e6
