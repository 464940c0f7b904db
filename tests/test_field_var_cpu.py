"""Pointwise predictive variance of the field evaluator (gmrf_eval_pairs / _var_batch / _calibration_batch, `FieldEvaluator.pairs`,
`pair_pattern`, `variance`, `calibration`): what can be checked without a GPU, on handles created with device = -1 -- the
declarations, the pair table's structure and completeness, and that the pairs of the loops' workloads pass the selected inverse's
pattern rule under those workloads' block partitions."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from tests import field_eval_oracle as FO
from tests import field_var_oracle as VO
from tests.test_host_logic import _check_julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["gmrf_eval_pairs", "gmrf_eval_var_batch", "gmrf_eval_calibration_batch"]
GEOMETRIES = [("line",) + g for g in FO.LINES] + [("tri",) + g for g in FO.TRIANGLES]
IDS = ["-".join(str(x) for x in g) for g in GEOMETRIES]
EPS = 2.0 ** -52


def case(pkg, geom):
    ev = VO.evaluator(pkg, geom, VO.points_of(geom), device=-1)
    return ev, ev.rows()


def test_new_exports_are_declared_everywhere(pkg, lib):
    hdr = open(os.path.join(ROOT, "include", "gmrf_hip.h")).read()
    shim = open(os.path.join(ROOT, "julia", "DiffEqGMRFsHIP.jl")).read()
    bound = _check_julia_ccalls(shim, hdr, 40)
    for name in NEW_EXPORTS:
        assert re.search(r"gmrf_status\s+%s\s*\(" % name, hdr), name
        assert name in pkg._cabi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
        assert name in bound, name
    for meth in ("pairs", "pair_pattern", "variance", "calibration"):
        assert hasattr(pkg.FieldEvaluator, meth)
    kernels = open(os.path.join(ROOT, "diffeqgmrfs.jl_amd", "csrc", "field_eval.hpp")).read()
    for kernel in ("field_eval_var", "field_eval_calibration_part"):
        assert re.search(r"__global__[^;{]*\b%s\s*\(" % kernel, kernels), kernel


@pytest.mark.parametrize("geom", GEOMETRIES, ids=IDS)
def test_pair_table_structure(pkg, geom):
    ev, (idx, w) = case(pkg, geom)
    P, pos = ev.pairs()
    W, ns = ev.width, ev.ns
    assert P.shape == (ns, ns) and P.has_canonical_format and np.all(P.data == 1.0)
    assert pos.dtype == np.int32 and pos.shape == (W * (W + 1) // 2, ev.npts)
    assert (P != P.T).nnz == 0                                                    # symmetric, both triangles stored
    assert np.all(np.diff(P.indptr) >= 0)
    for r in range(ns):                                                           # sorted, no duplicates
        assert np.all(np.diff(P.indices[P.indptr[r]:P.indptr[r + 1]]) > 0)
    # exactly the pairs some point uses (the diagonal of every dof used among them)
    used = np.zeros((ns, ns), dtype=bool)
    used[idx[:, :, None], idx[:, None, :]] = True
    assert np.array_equal(P.toarray() != 0.0, used)
    assert np.array_equal(P.diagonal() != 0.0, np.isin(np.arange(ns), idx))
    # pos addresses the entry (idx_a, idx_b), a >= b, for every point
    rows = np.repeat(np.arange(ns), np.diff(P.indptr))
    for a in range(W):
        for b in range(a + 1):
            k = pos[a * (a + 1) // 2 + b]
            assert k.min() >= 0 and k.max() < P.nnz
            assert np.array_equal(rows[k], idx[:, a]) and np.array_equal(P.indices[k], idx[:, b]), (a, b)
    if geom[0] == "line" and geom[3] == "periodic":
        # the wrap cell (the last point lies in it) pairs dof ns - 1 with dof 0
        assert idx[-1, 0] == 0 and idx[-1, -1] == ns - 1
        assert P[ns - 1, 0] == 1.0 and P[0, ns - 1] == 1.0
        k = pos[(W - 1) * W // 2, -1]
        assert rows[k] == ns - 1 and P.indices[k] == 0
    ev.close()


def test_pair_pattern_is_the_kronecker_product(pkg):
    ev, _ = case(pkg, ("line", 5, 2, "periodic"))
    P, _ = ev.pairs()
    assert (ev.pair_pattern() != P).nnz == 0 and ev.pair_pattern().nnz == P.nnz
    for nt in (2, 3):
        K = ev.pair_pattern(nt)
        want = sp.kron(sp.identity(nt), P, format="csr")
        want.sort_indices()
        assert K.shape == (nt * ev.ns, nt * ev.ns) and K.has_sorted_indices
        assert np.array_equal(K.indptr, want.indptr) and np.array_equal(K.indices, want.indices)
        # slice t's copy of entry e sits at t nnz(P) + e
        for t in range(nt):
            assert np.array_equal(K.indices[t * P.nnz:(t + 1) * P.nnz], P.indices + t * ev.ns)
    with pytest.raises(ValueError):
        ev.pair_pattern(0)
    ev.close()


@pytest.mark.parametrize("geom", GEOMETRIES, ids=IDS)
def test_pair_table_is_complete(pkg, geom):
    """diag(E Sigma E^T) through matrix() and a dense SPD Sigma in longdouble equals the quadratic form over the pair table's
    entries alone, to 4 eps (longdouble) relative: an omitted or misplaced pair is wrong by O(1)."""
    ev, (idx, w) = case(pkg, geom)
    P, pos = ev.pairs()
    ns, W = ev.ns, ev.width
    rng = np.random.default_rng(11)
    G = rng.standard_normal((ns, ns)).astype(np.longdouble)
    Sigma = G @ G.T + ns * np.eye(ns, dtype=np.longdouble)
    E = ev.matrix().toarray().astype(np.longdouble)
    want = np.sum((E @ Sigma) * E, axis=1)
    rows = np.repeat(np.arange(ns), np.diff(P.indptr))
    vals = Sigma[rows, P.indices]                                                  # Sigma on P, in its CSR order
    wl = w.astype(np.longdouble)
    got = np.zeros(ev.npts, dtype=np.longdouble)
    for a in range(W):
        for b in range(W):
            hi, lo = max(a, b), min(a, b)
            got += wl[:, a] * wl[:, b] * vals[pos[hi * (hi + 1) // 2 + lo]]
    rel = np.abs(got - want) / np.abs(want)                  # (Sigma >= ns I and sum w = 1: want >= ns / width, no cancellation to 0)
    print(f"{geom}: worst |pair form - diag(E Sigma E')| / |.| = {float(rel.max()):.2e} ({float(rel.max()) / EPS:.4f} eps)")
    assert np.all(rel <= 4 * EPS)
    ev.close()


def _symbolic_rmax(lib, pkg, Q, n_blocks):
    Q = sp.csc_matrix(Q)
    Q.sort_indices()
    cp, rv = Q.indptr.astype(np.int64), Q.indices.astype(np.int64)
    out = np.zeros(8, dtype=np.int64)
    assert lib.gmrf_test_symbolic_csc(Q.shape[0], n_blocks, pkg._cabi.ptr(cp), pkg._cabi.ptr(rv), 0, pkg._cabi.ptr(out)) == 0
    return int(out[1])


def _loop_workloads(pkg):
    Q0, obs, nb = pkg.workloads.darcy_conditioning(16)
    A = obs[0][0]
    yield "darcy_conditioning(16)", ("tri", 16, 16, 1), 1, (Q0 + 1e8 * (A.T @ A)).tocsc(), nb
    w = pkg.workloads.burgers(32, 6)
    yield "burgers32x6", ("line", 32, 1, "periodic"), 6, w.Q, w.n_blocks
    nc, nt = 16, 4
    ic = np.sin(2 * np.pi * np.arange(2 * nc) / (2 * nc))
    Qp, Aic, _ = pkg.workloads.burgers_line_prior_from_bulk(nc, nt, 1.0 / (nt - 1), 0.01 / math.pi, 0.3, ic, order=2, bc="periodic")
    yield "burgers_line_prior 16x4 P2", ("line", nc, 2, "periodic"), nt, (Qp + 1e8 * (Aic.T @ Aic)).tocsc(), nt


def test_the_loops_pairs_pass_the_selected_inverses_pattern_rule(pkg, lib):
    """Every pair of 300 seeded random points + the corner cases lies in the same or a neighbouring block of the workload's
    partition, and a pair across two blocks has its later index below the rmax the symbolic phase reports for that Q."""
    for name, geom, nt, Q, nb in _loop_workloads(pkg):
        ev, _ = case(pkg, geom)
        n = nt * ev.ns
        assert Q.shape == (n, n) and n % nb == 0, name
        bs, rmax = n // nb, _symbolic_rmax(lib, pkg, Q, nb)
        K = ev.pair_pattern(nt).tocoo()
        br, bc = K.row // bs, K.col // bs
        assert np.all(np.abs(br - bc) <= 1), name
        cross = br != bc
        later = np.where(br > bc, K.row % bs, K.col % bs)[cross]
        print(f"{name}: {K.nnz} pair entries, {int(cross.sum())} across blocks, largest later index "
              f"{int(later.max()) if later.size else -1}, rmax {rmax}, block size {bs}")
        assert np.all(later < rmax), name
        if geom[0] == "tri":
            assert cross.any()                                                     # (the rule is exercised, not vacuous)
        ev.close()


def test_numeric_calls_need_the_device(pkg, lib):
    ev, _ = case(pkg, ("line", 4, 1, "periodic"))
    F = C.c_void_p(1)                    # never followed: the evaluator is refused first

    class Fake:
        _h, batch = F, 1
    for call in (lambda: ev.variance(Fake), lambda: ev.calibration(Fake, np.zeros((1, ev.ns)), np.ones((1, ev.npts)))):
        with pytest.raises(pkg.GmrfError) as e:
            call()
        assert e.value.status == pkg._cabi.ERR_NO_DEVICE
    assert lib.gmrf_eval_pairs(None, None, None, None, None) == pkg._cabi.ERR_BAD_SHAPE
    ev.close()
