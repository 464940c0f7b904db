"""The selected-inverse oracle (tests/selinv_oracle.py) against the dense inverse, without a GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import bt_oracle as O
from tests import selinv_oracle as SI


def _check(Q, n_blocks, tol=1e-12):
    Q = sp.csr_matrix(Q)
    F = O.tridiagonal_cholesky(Q, n_blocks)
    Sigma = np.linalg.inv(Q.toarray())
    d = np.sqrt(np.diag(Sigma))
    vals, mask, scale = SI.pattern_values(F, Q)
    assert mask.all()
    rows = np.repeat(np.arange(Q.shape[0]), np.diff(Q.indptr))
    want = Sigma[rows, Q.indices]
    assert np.allclose(scale, d[rows] * d[Q.indices], rtol=1e-12)
    assert SI.entry_error(vals, want, scale) <= tol
    # the whole blocks too, not only the pattern entries
    diag, low = SI.selected_blocks(F)
    bs = F.block_size
    for i in range(n_blocks):
        s = slice(i * bs, (i + 1) * bs)
        assert np.max(np.abs(diag[i] - Sigma[s, s])) <= tol * np.max(np.abs(Sigma[s, s]))
        if i + 1 < n_blocks:
            t = slice((i + 1) * bs, (i + 2) * bs)
            assert np.max(np.abs(low[i] - Sigma[t, s])) <= tol * np.max(np.abs(Sigma[s, s]))
    return F


@pytest.mark.parametrize("bs,n_blocks", [(7, 5), (100, 3), (64, 4)])
def test_oracle_random_block_tridiagonal(pkg, bs, n_blocks):
    w = pkg.workloads.random_block_tridiagonal(n_blocks, bs, seed=3)
    _check(w.Q, n_blocks)


def test_oracle_ar1_kron_identity(pkg):
    w = pkg.workloads.ar1_chain_kron_identity(6, 40, phi=0.6)
    _check(w.Q, w.n_blocks)


def test_oracle_laplace_grid(pkg):
    w = pkg.workloads.laplace_kappa_grid(30, 9, kappa2=0.5)
    _check(w.Q, w.n_blocks)
    # the diagonal against the closed form
    F = O.tridiagonal_cholesky(w.Q, w.n_blocks)
    diag, _ = SI.selected_blocks(F)
    v = np.concatenate([np.diag(diag[i]) for i in range(w.n_blocks)])
    assert np.max(np.abs(v / pkg.workloads.laplace_kappa_grid_variances(30, 9, 0.5) - 1.0)) < 1e-12


def test_oracle_last_blocks_and_mask(pkg):
    w = pkg.workloads.random_block_tridiagonal(5, 50, seed=8)
    F = O.tridiagonal_cholesky(w.Q, w.n_blocks)
    Q = sp.csr_matrix(w.Q)
    vals, mask, scale = SI.pattern_values(F, Q, last_blocks=2)
    rows = np.repeat(np.arange(Q.shape[0]), np.diff(Q.indptr))
    reached = (rows >= 150) & (Q.indices >= 150)
    assert np.array_equal(mask, reached)
    Sigma = np.linalg.inv(Q.toarray())
    assert SI.entry_error(vals, Sigma[rows, Q.indices], scale, mask) < 1e-12
