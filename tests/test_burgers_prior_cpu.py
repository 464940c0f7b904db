"""The Burgers prior without a GPU: the structural pattern of `BurgersP1Prior` (device = -1), the one statement of the prior in
`workloads.burgers_prior_from_bulk`, and -- on the CPU, in NumPy -- that the stencil form the device kernels evaluate meets the
tolerance tests/test_gpu_burgers_prior.py holds the device to."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import burgers_prior_checks as BP


def _prior(pkg, ns, nt, device=-1):
    return pkg.BurgersP1Prior(ns, nt, 1.0 / (nt - 1), BP.NU, ic_noise=BP.IC_NOISE, device=device)


@pytest.mark.parametrize("ns,nt", [(64, 8), (40, 5), (5, 2)])
def test_pattern_is_symmetric_sorted_and_block_tridiagonal(pkg, ns, nt):
    P = _prior(pkg, ns, nt).pattern
    n = ns * nt
    assert P.shape == (n, n) and P.nnz == (11 * nt - 6) * ns and P.has_sorted_indices
    assert all(np.all(np.diff(P.indices[P.indptr[j]:P.indptr[j + 1]]) > 0) for j in range(n))        # ascending, no duplicates
    assert abs(P - P.T).nnz == 0
    assert pkg.workloads.block_bandwidth_ok(P, nt)
    C = P.tocoo()
    counts = np.zeros((nt, nt), dtype=np.int64)
    np.add.at(counts, (C.row // ns, C.col // ns), 1)
    for t in range(nt):
        assert counts[t, t] == 5 * ns
        if t > 0:
            assert counts[t, t - 1] == 3 * ns and counts[t - 1, t] == 3 * ns
    # the offsets: 0, +-1, +-2 in the diagonal blocks, 0, +-1 beside them (periodic)
    d = (C.row % ns - C.col % ns) % ns
    same = C.row // ns == C.col // ns
    assert set(d[same].tolist()) == {0, 1, 2, ns - 1, ns - 2} and set(d[~same].tolist()) == {0, 1, ns - 1}


@pytest.mark.parametrize("ns,nt", [(64, 8), (40, 5)])
def test_pattern_contains_the_workloads_pattern(pkg, ns, nt):
    P = _prior(pkg, ns, nt).pattern
    ics = pkg.workloads.burgers_initial_conditions(ns, 2)
    for ic in ics:
        Q = pkg.workloads.burgers(ns, nt, BP.IC_NOISE, 0.0, ic).Q.copy()
        Q.eliminate_zeros()
        Q.data[:] = 1.0
        assert (Q - Q.multiply(P)).nnz == 0 and abs(Q - Q.multiply(P)).sum() == 0.0
        print(f"{ns}x{nt}: workload nnz {Q.nnz}, structural nnz {P.nnz}")


def test_four_nodes_fold_the_offsets(pkg):
    with pytest.raises(pkg.GmrfError) as e:
        _prior(pkg, 4, 5)
    assert e.value.status == pkg._cabi.ERR_BAD_SHAPE and "ns >= 5" in str(e.value)
    with pytest.raises(pkg.GmrfError) as e:        # the numeric phase needs the GPU: no CPU fallback
        _prior(pkg, 8, 3).values_batch(np.zeros((2, 8)))
    assert e.value.status == pkg._cabi.ERR_NO_DEVICE


@pytest.mark.parametrize("p", [0, 2])
def test_prior_from_bulk_is_the_prior_of_burgers(pkg, p):
    W = pkg.workloads
    ns, nt = 64, 8
    ic = W.burgers_initial_conditions(ns, 3)[p]
    w = W.burgers(ns, nt, BP.IC_NOISE, 0.0, ic)
    Q, _, rhs = BP.oracle(W, ns, nt, ic.mean(), ic)
    D = (w.Q - Q).tocsc()
    D.eliminate_zeros()
    assert D.nnz == 0
    assert np.array_equal(rhs, w.rhs)


@pytest.mark.parametrize("ns,nt,B", [(64, 8, 5), (40, 5, 3)])
def test_stencil_form_meets_the_value_tolerance(pkg, ns, nt, B):
    """The arithmetic of csrc/burgers_prior.hpp, written in NumPy, against the oracle within the bound the device is held to."""
    W = pkg.workloads
    P = _prior(pkg, ns, nt).pattern
    ics = BP.initial_conditions(W, ns, B)
    for p in range(B):
        bulk = float(ics[p].mean())
        Q, Qp, rhs = BP.oracle(W, ns, nt, bulk, ics[p])
        S = BP.stencil_matrix(P, ns, nt, 1.0 / (nt - 1), BP.NU, BP.IC_NOISE, bulk)
        assert abs(S - S.T).nnz == 0                                  # bitwise symmetric
        ev = BP.value_excess(S, Q, ns, nt)
        er = BP.rhs_excess(BP.stencil_rhs(ns, nt, 1.0 / (nt - 1), BP.NU, BP.IC_NOISE, bulk, ics[p]), rhs, Qp, ns, bulk, ics[p])
        print(f"{ns}x{nt} p={p}: values at {ev:.3f} of the bound, Qx_prior at {er:.3f}")
        assert ev <= 1.0 and er <= 1.0
    # a wrong coefficient is far outside: the sign of the advection term (the last problem's bulk speed is not zero)
    assert abs(bulk) > 0.1
    bad = BP.stencil_matrix(P, ns, nt, 1.0 / (nt - 1), BP.NU, BP.IC_NOISE, -bulk)
    assert BP.value_excess(bad, Q, ns, nt) > 1e6
