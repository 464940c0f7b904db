"""The twisted-order oracle (tests/twisted_oracle.py) against the reference-order oracle, on the CPU: T T^T = Q, and the
order-invariant quantities (mean, marginal variances, log-determinant) agree."""
import numpy as np
import pytest

from oracle import bt_oracle as O
from tests import twisted_oracle as TW


def _cases(pkg):
    W = pkg.workloads
    return [W.random_block_tridiagonal(7, 12, seed=3), W.random_block_tridiagonal(5, 8, seed=11, density=0.5),
            W.darcy(16)]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_twisted_oracle_factors_q(pkg, which):
    w = _cases(pkg)[which]
    N = w.n_blocks
    Q = w.Q.toarray()
    Fo = O.tridiagonal_cholesky(w.Q, N)
    mu_o = O.ldiv(Fo, w.rhs)
    var_o = O.marginal_variances_exact(Fo)
    ld_o = O.logdet(Fo)
    for m in sorted({0, 1, N // 2, N - 2, N - 1}):
        F = TW.tridiagonal_cholesky(w.Q, N, m)
        T = TW.dense_T(F)
        assert np.linalg.norm(T @ T.T - Q) / np.linalg.norm(Q) < 1e-13, m
        bs = F.block_size
        for i in range(N):                                     # lower (i <= m) / upper (i > m) diagonal blocks
            D = F.diag[i]
            assert np.allclose(np.triu(D, 1) if i <= m else np.tril(D, -1), 0.0)
        assert np.linalg.norm(TW.ldiv(F, w.rhs) - mu_o) / np.linalg.norm(mu_o) < 1e-11
        assert np.max(np.abs(TW.marginal_variances_exact(F) - var_o) / var_o) < 1e-10
        assert abs(TW.logdet(F) - ld_o) <= 1e-11 * abs(ld_o) + 1e-10
        b = np.random.default_rng(m).standard_normal(w.n)
        assert np.allclose(T @ TW.forward_solve(F, b), b, rtol=0, atol=1e-9 * np.abs(b).max())
        assert np.allclose(T.T @ TW.backward_solve(F, b), b, rtol=0, atol=1e-9 * np.abs(b).max())
        if m == N - 1:                                         # no bottom chain: the reference order itself
            for i in range(N):
                assert np.array_equal(F.diag[i], Fo.chos[i])
        assert bs * N == w.n


def test_twisted_oracle_sample_covariance_is_q_inverse(pkg):
    """T^-T z has covariance T^-T T^-1 = Q^-1 whatever the order: exactly, on the whole identity."""
    w = pkg.workloads.random_block_tridiagonal(6, 8, seed=5)
    F = TW.tridiagonal_cholesky(w.Q, w.n_blocks, 2)
    X = TW.backward_solve(F, np.eye(w.n))
    Qi = np.linalg.inv(w.Q.toarray())
    assert np.linalg.norm(X @ X.T - Qi) / np.linalg.norm(Qi) < 1e-12
