"""The Burgers line tangent over (order, scheme, bc) without a GPU: the library's patterns (device -1) and rejections, the
restatement tests/burgers_cn_oracle.py checked against itself and against oracle/bt_oracle.py, and the benchmark
_research/burgers_chen24.jl (workloads.burgers_chen24_batch) run on the restatement alone."""
import ctypes as C
import itertools

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import bt_oracle as O
from tests import burgers_cn_oracle as BO
from tests import gn_batch_oracle as GO

COMBOS = list(itertools.product((1, 2), ("euler", "cn"), ("periodic", "dirichlet")))
DT, NU, LENGTH = 0.05, 0.01, 2.0


def shapes(bc):
    """The smallest mesh the bc admits (3 cells periodic, 2 dirichlet) on 2 slices, and 5 cells x 4 slices."""
    return ((3 if bc == "periodic" else 2, 2), (5, 4))


def dofs(nc, order, bc):
    return order * nc + (1 if bc == "dirichlet" else 0)


@pytest.fixture(scope="module")
def chen(pkg):
    """BO.CHEN_CASE under both schemes, computed once and left unchanged: scheme -> (workload, fJ, batch_loop result)."""
    return {s: BO.chen_case(pkg.workloads, s) for s in ("cn", "euler")}


@pytest.mark.parametrize("order,scheme,bc", COMBOS)
def test_pattern_is_the_oracles(pkg, order, scheme, bc):
    rng = np.random.default_rng(1)
    for nc, nt in shapes(bc):
        ns = dofs(nc, order, bc)
        b = pkg.BurgersP1Tangent(ns, nt, DT, NU, device=-1, order=order, scheme=scheme, bc=bc, length=LENGTH)
        _, J = BO.f_and_J(nc, nt, DT, NU, rng.standard_normal(ns * nt), order, scheme, bc, LENGTH)
        assert b.cells == nc and b.pattern.shape == J.shape == ((nt - 1) * ns, nt * ns) and b.nnz == J.nnz
        assert np.array_equal(b.pattern.indptr, J.indptr) and np.array_equal(b.pattern.indices, J.indices)
        assert J.has_sorted_indices
        # a row holds its window's in-range columns: clipped at the two ends of the Dirichlet interval only
        per_row = np.diff(J.indptr).reshape(nt - 1, ns)[0] // 2
        full = np.array([5 if (order == 2 and i % 2 == 0) else 3 for i in range(ns)])
        if bc == "dirichlet":
            full[0] = full[-1] = order + 1
        assert np.array_equal(per_row, full)


def test_old_entry_points_forward_to_the_common_creator(pkg):
    """gmrf_burgers_p1_create / _p2_create against the euler / periodic pattern of the new constructor."""
    lib = pkg._cabi.load()
    for order, create in ((1, lib.gmrf_burgers_p1_create), (2, lib.gmrf_burgers_p2_create)):
        ns, nt = 6 * order, 3
        h = C.c_void_p()
        pkg._cabi.check(create(-1, None, ns, nt, DT, NU, C.byref(h)))
        nnz = C.c_int64(0)
        pkg._cabi.check(lib.gmrf_burgers_p1_pattern(h, C.byref(nnz), None, None, 0))
        b = pkg.BurgersP1Tangent(ns, nt, DT, NU, device=-1, order=order)
        rp, ci = np.empty(b.rows + 1, dtype=np.int64), np.empty(nnz.value, dtype=np.int64)
        pkg._cabi.check(lib.gmrf_burgers_p1_pattern(h, None, pkg._cabi.ptr(rp), pkg._cabi.ptr(ci), 0))
        lib.gmrf_burgers_p1_destroy(h)
        assert nnz.value == b.nnz and np.array_equal(rp, b.pattern.indptr) and np.array_equal(ci, b.pattern.indices)


def test_bad_shapes_are_refused(pkg):
    cabi = pkg._cabi
    lib = cabi.load()

    def create(nc=5, nt=4, dt=DT, nu=NU, order=1, scheme=0, bc=0, length=1.0):
        h = C.c_void_p()
        st = lib.gmrf_burgers_line_create(-1, None, nc, nt, dt, nu, order, scheme, bc, length, C.byref(h))
        if h.value:
            lib.gmrf_burgers_p1_destroy(h)
        return st

    assert create() == 0 and create(order=2, scheme=1, bc=1, length=2.0) == 0
    assert create(nc=2, bc=1) == 0 and create(nc=3, bc=0) == 0
    for bad in (dict(scheme=2), dict(scheme=-1), dict(bc=2), dict(bc=-1), dict(order=0), dict(order=3), dict(length=0.0),
                dict(length=-1.0), dict(length=float("nan")), dict(nc=1, bc=1), dict(nc=2, bc=0), dict(nt=1), dict(dt=0.0)):
        assert create(**bad) == cabi.ERR_BAD_SHAPE, bad
    assert lib.gmrf_burgers_line_create(-1, None, 5, 4, DT, NU, 1, 0, 0, 1.0, None) == cabi.ERR_BAD_SHAPE

    def refused(**kw):
        with pytest.raises(pkg.GmrfError) as e:
            pkg.BurgersP1Tangent(kw.pop("ns", 11), 4, DT, NU, device=-1, **kw)
        assert e.value.status == cabi.ERR_BAD_SHAPE
        return str(e.value)

    refused(scheme="rk4")
    refused(bc="neumann")
    refused(order=3)
    refused(length=0.0)
    # the parity of ns: 2 cells + 1 on the quadratic Dirichlet interval, 2 cells on the quadratic periodic line
    assert "cells" in refused(ns=10, order=2, bc="dirichlet") and "cells" in refused(ns=11, order=2, bc="periodic")
    refused(ns=3, order=2, bc="dirichlet")              # one quadratic cell
    refused(ns=2, order=1, bc="dirichlet")              # one P1 cell
    for ns, kw in ((11, dict(order=2, bc="dirichlet")), (10, dict(order=2)), (10, dict(bc="dirichlet")), (3, dict(bc="dirichlet"))):
        assert pkg.BurgersP1Tangent(ns, 4, DT, NU, device=-1, **kw).ns == ns


@pytest.mark.parametrize("order,scheme,bc", COMBOS)
def test_oracle_tangent_is_the_derivative_of_its_residual(order, scheme, bc):
    """f is quadratic in w, so the central difference of f with ANY step is J(w) d up to rounding.  On the Dirichlet interval
    the prescribed columns of J are zero while the cells still read w there (the reference passes the prescribed value), so d
    vanishes at the prescribed dofs.  The error is measured against max |J d|; the largest seen over the 16 cases here is
    3.6e-16 (a few roundings of sums of O(1) terms), the bound one decade above."""
    rng = np.random.default_rng(3)
    for nc, nt in shapes(bc):
        ns = dofs(nc, order, bc)
        w, d = rng.standard_normal(ns * nt), rng.standard_normal(ns * nt)
        if bc == "dirichlet":
            d.reshape(nt, ns)[:, [0, -1]] = 0.0
        f, J = BO.f_and_J(nc, nt, DT, NU, w, order, scheme, bc, LENGTH)
        fp, _ = BO.f_and_J(nc, nt, DT, NU, w + d, order, scheme, bc, LENGTH)
        fm, _ = BO.f_and_J(nc, nt, DT, NU, w - d, order, scheme, bc, LENGTH)
        jd = J @ d
        err = np.max(np.abs(jd - 0.5 * (fp - fm))) / np.max(np.abs(jd))
        print(f"order {order} {scheme} {bc} {nc}x{nt}: {err:.2e}")
        assert err < 4e-15
        if bc == "dirichlet":                           # prescribed rows and columns: stored zeros
            Jd = J.toarray().reshape(nt - 1, ns, nt, ns)
            assert not np.any(Jd[:, [0, -1]]) and not np.any(Jd[:, :, :, [0, -1]]) and not np.any(f.reshape(nt - 1, ns)[:, [0, -1]])
            assert np.all(Jd[np.arange(nt - 1), 1, np.arange(1, nt), 1] != 0.0)


@pytest.mark.parametrize("order", (1, 2))
def test_euler_periodic_oracle_is_the_existing_oracle(order):
    """Against oracle.bt_oracle.burgers_f_and_J (cell by cell, scalar): the same pattern; values and f to a few roundings of
    their scale (two summation orders of the same terms)."""
    rng = np.random.default_rng(4)
    for nc, nt in ((3, 2), (5, 4), (9, 3)):
        ns = order * nc
        w = rng.standard_normal(ns * nt)
        f, J = BO.f_and_J(nc, nt, DT, NU, w, order, "euler", "periodic", 1.0)
        fo, Jo = O.burgers_f_and_J(ns, nt, DT, NU, w, order)
        assert np.array_equal(J.indptr, Jo.indptr) and np.array_equal(J.indices, Jo.indices)
        assert np.max(np.abs(J.data - Jo.data)) <= 4 * np.finfo(float).eps * np.max(np.abs(Jo.data))
        assert np.max(np.abs(f - fo)) <= 8 * np.finfo(float).eps * max(np.max(np.abs(fo)), 1.0)


def test_euler_tie_on_the_oracle(pkg):
    """J_cn[:, t] = (J_euler[:, t] + M) / 2, and for t >= 2 J_cn[block t, t-1] = J_euler[block t-1, t-1] / 2 - 3/2 M, with M read
    off the Euler tangent (-J_euler[block t, t-1])."""
    rng = np.random.default_rng(5)
    for order, bc in itertools.product((1, 2), ("periodic", "dirichlet")):
        nc, nt = 5, 4
        ns = dofs(nc, order, bc)
        w = rng.standard_normal(ns * nt)
        Je = BO.f_and_J(nc, nt, DT, NU, w, order, "euler", bc, LENGTH)[1].toarray().reshape(nt - 1, ns, nt, ns)
        Jc = BO.f_and_J(nc, nt, DT, NU, w, order, "cn", bc, LENGTH)[1].toarray().reshape(nt - 1, ns, nt, ns)
        M = -Je[0, :, 0, :]
        for t in range(1, nt):
            assert np.max(np.abs(Jc[t - 1, :, t, :] - 0.5 * (Je[t - 1, :, t, :] + M))) < 1e-15
            if t >= 2:
                assert np.max(np.abs(Jc[t - 1, :, t - 1, :] - (0.5 * Je[t - 2, :, t - 1, :] - 1.5 * M))) < 1e-15


def test_workload_and_cole_hopf(pkg):
    W = pkg.workloads
    c = BO.CHEN_CASE
    w = W.burgers_chen24_batch(c["nc"], c["nt"], c["B"], c["nu"], c["amps"])
    ns = 2 * c["nc"] + 1
    assert w["ns"] == ns == 65 and w["n"] == 1690 and w["m"] == 1625 and w["n_blocks"] == 26 and w["truth"].shape == (3, ns)
    assert w["Q"].shape == (1690, 1690) and W.block_bandwidth_ok(w["Q"], w["n_blocks"]) and abs(w["Q"] - w["Q"].T).max() == 0.0
    assert np.array_equal(w["xs"], -1.0 + 2.0 * np.arange(ns) / (ns - 1)) and np.array_equal(w["x0"], w["x_prior"])
    assert np.array_equal(w["ic"][1, 1:-1], -0.5 * np.sin(np.pi * w["xs"])[1:-1]) and not np.any(w["ic"][:, [0, -1]])
    # the start point carries the initial condition at the interior dofs of slice 0 (observed with 1e12) and ends pinned by 1e8
    assert np.max(np.abs((w["x0"][:, :ns] - w["ic"])[:, 1:-1])) < 1e-6 and np.max(np.abs(w["x0"].reshape(3, 26, ns)[:, :, [0, -1]])) < 1e-3
    for p in range(3):
        assert np.max(np.abs(w["Q"] @ w["x_prior"][p] - w["Qx_prior"][p])) < 1e-3 * np.max(np.abs(w["Qx_prior"][p]))
    # Cole-Hopf: t -> 0 gives the initial condition; the amplitude form is odd in x and scales as u(x, t; a, nu) = a u(x, a t; 1, nu / a)
    xs = w["xs"]
    for a in c["amps"]:
        assert np.max(np.abs(W.burgers_cole_hopf(xs, 1e-12, 0.02, a) + a * np.sin(np.pi * xs))) < 1e-5
        u = W.burgers_cole_hopf(xs, 1.0, 0.02, a)
        assert np.max(np.abs(u + u[::-1])) < 1e-13
        assert np.max(np.abs(u - a * W.burgers_cole_hopf(xs, a * 1.0, 0.02 / a, 1.0))) < 1e-12
    with pytest.raises(ValueError):
        W.burgers_chen24_batch(32, 26, 2, 0.02, (1.0, 0.5, 1.3))


def test_loop_reproduces_the_benchmark_table(chen):
    """The Gauss-Newton loop on the restatement against Cole-Hopf at T = 1, nu = 0.02, 32 quadratic cells x 26 slices, amplitudes
    (1.0, 0.5, 1.3).  Measured: Crank-Nicolson rel_err 1.448e-3, 3.76e-4, 1.940e-3 in 6, 5, 6 steps; implicit Euler 2.686e-2,
    1.387e-2, 4.063e-2 in 6, 5, 6 steps; ratios 0.054, 0.027, 0.048."""
    w, _, (x, steps, hist, rels, _) = chen["cn"]
    we, _, (xe, steps_e, _, rels_e, _) = chen["euler"]
    cn, eu = BO.last_slice_rel_err(w, x), BO.last_slice_rel_err(we, xe)
    print("cn", cn, steps, "euler", eu, steps_e, "ratio", cn / eu, "stop margin", GO.stop_margin(rels, BO.CHEN_CASE["rtol"]))
    assert np.all(cn < 0.2 * eu)
    assert len(set(steps.tolist())) >= 2 and steps.max() < BO.CHEN_CASE["max_steps"]
    # every stop decision of the case is at least a factor 3 from the threshold: the device's step counts can be compared exactly
    assert GO.stop_margin(rels, BO.CHEN_CASE["rtol"]) > 3.0 and GO.stop_margin(rels_e, BO.CHEN_CASE["rtol"]) > 3.0
    for p in range(3):
        assert np.all(np.diff(hist[p, :steps[p] + 1])[-2:] < 0.0)


def test_posterior_is_block_tridiagonal_and_factors(pkg, chen):
    """Q + noise J'J at the final iterate, time-major with nt blocks: inside the block tri-band, and positive definite for the
    block-tridiagonal oracle at the workload's fidelity noise 1e12."""
    w, fJ, (x, _, _, _, _) = chen["cn"]
    for p in range(3):
        _, J = fJ(x[p])
        A = BO.posterior_matrix(w["Q"], J, w["noise"])
        assert pkg.workloads.block_bandwidth_ok(A, w["n_blocks"])
        F = O.tridiagonal_cholesky(A, w["n_blocks"])
        b = np.cos(np.arange(w["n"]))
        r = np.linalg.norm(A @ O.ldiv(F, b) - b) / np.linalg.norm(b)
        ld, ld_lu = O.logdet(F), BO.logdet(A)
        print(f"p={p}: residual of a solve {r:.2e}, logdet {ld:.12e} SuperLU {ld_lu:.12e}")
        assert r < 1e-9 and abs(ld - ld_lu) <= 1e-10 * abs(ld_lu)
