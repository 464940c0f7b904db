"""The symbolic phase's envelope bounds (host only: gmrf_test_envelope_csc) against their restatement from the SciPy pattern
(tests/envelope_ref.py), and the K units the bounds leave of darcy256's first panel: 312 -> 244 for the rank-256 update, 120 -> 90
for the panel product, 99 with the forward solve's tail row riding in its last row tile."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from tests import envelope_ref as E


def hook(pkg, lib, Q, N):
    Q = sp.csc_matrix(Q)
    Q.sort_indices()
    cp, rv = Q.indptr.astype(np.int64), Q.indices.astype(np.int64)
    n = C.c_int64(0)
    pkg._cabi.check(lib.gmrf_test_envelope_csc(Q.shape[0], N, pkg._cabi.ptr(cp), pkg._cabi.ptr(rv), 0, None, None, None, 0, C.byref(n)))
    if n.value == 0:
        return None
    nt = n.value // N
    lo, hi = np.zeros(n.value, np.int32), np.zeros(n.value, np.int32)
    un = np.zeros(N * (nt // 4) * 3)
    pkg._cabi.check(lib.gmrf_test_envelope_csc(Q.shape[0], N, pkg._cabi.ptr(cp), pkg._cabi.ptr(rv), 0, pkg._cabi.ptr(lo), pkg._cabi.ptr(hi),
                                               pkg._cabi.ptr(un), n.value, C.byref(n)))
    return lo.reshape(N, nt), hi.reshape(N, nt), un.reshape(N, nt // 4, 3)


@pytest.fixture(scope="module")
def darcy(pkg):
    out = {}
    for nxy in (128, 256):
        w = pkg.workloads.darcy(nxy)
        out[nxy] = (w, hook(pkg, pkg._cabi.load(), w.Q, w.n_blocks), E.envelope(w.Q, w.n_blocks))
    return out


@pytest.mark.parametrize("nxy", [128, 256])
def test_darcy_bounds_match_the_pattern(darcy, nxy):
    w, (lo, hi, un), (lo_py, hi_py) = darcy[nxy]
    assert np.array_equal(lo, lo_py) and np.array_equal(hi, hi_py)
    N, nt = lo.shape
    q = nt // 4                      # 64-row tiles per mesh row; the last mesh row of a block meets the first
    for i in (1, 5, N - 1):
        assert list(lo[i, :3 * q]) == [0] * (3 * q) and list(hi[i, :3 * q]) == [64 * nt] * (3 * q)
        assert list(lo[i, 3 * q:]) == [64 * k for k in range(q)]
        # darcy256: a panel is one mesh row, and the row tiles meet one 64-column chunk of it each; darcy128: a panel is two mesh
        # rows, and the last mesh row meets the second of them as well
        assert list(hi[i, 3 * q:]) == ([64 * (k + 1) for k in range(q)] if nxy == 256 else [256] * q)
    for i in range(N):
        for p in range(nt // 4):
            assert (un[i, p, 0], un[i, p, 2]) == E.units(lo_py, hi_py, i, p, False)
            assert un[i, p, 1] == E.units(lo_py, hi_py, i, p, True)[0]


def test_darcy256_units(darcy):
    w, (lo, hi, un), _ = darcy[256]
    for i in (1, 5, 63):
        assert list(un[i, 0]) == [90.0, 99.0, 244.0]
        # the later panels: as without the bounds
        for p in (1, 2):
            m3 = 16 - 4 * p - 4
            assert list(un[i, p]) == [10.0 * m3, 10.0 * m3, 4.0 * m3 * (m3 + 1) / 2]


def test_trivial_bounds_and_odd_blocks(pkg, lib):
    Q = E.no_structure_chain()
    lo, hi, un = hook(pkg, lib, Q, 3)
    lo_py, hi_py = E.envelope(Q, 3)
    assert np.array_equal(lo, lo_py) and np.array_equal(hi, hi_py)
    assert list(un[:, 0].ravel()) == [40.0, 40.0, 40.0] * 3
    # blocks of 192 (padded to 256) have one panel and nothing below it; blocks of 128 are no multiple of 256: no bounds
    Q1 = sp.csc_matrix(sp.diags([-np.ones(383), 4.0 * np.ones(384), -np.ones(383)], [-1, 0, 1]))
    lo, hi, un = hook(pkg, lib, Q1, 2)
    assert np.array_equal(lo, E.envelope(Q1, 2)[0]) and not un.any()
    assert hook(pkg, lib, sp.csc_matrix(Q1[:256, :256]), 2) is None
