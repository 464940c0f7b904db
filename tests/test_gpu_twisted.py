"""GPU tests of the twisted (two-ended) elimination order (gmrf_bt_set_order): order-invariant results against the
reference-order oracle (oracle/bt_oracle.py), order-specific ones (blocks of T, half-solves, samples for a given z)
against the twisted oracle (tests/twisted_oracle.py).  Tolerances as in tests/test_gpu_parity.py."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import bt_oracle as O
from tests import twisted_oracle as TW
from tests.test_gpu_parity import EPS, TOL_FACTOR, rel, solve_tol

pytestmark = pytest.mark.gpu

VAR_TOL = 1e-9


def _var_tol(w):
    return max(VAR_TOL, 4.0 * solve_tol(w))


def _twisted(pkg, w, meet=None):
    F = pkg.TridiagonalCholeskyFactor(order="twisted", meet=meet)
    F.factor(w.Q, w.n_blocks)
    return F


def _no_aborts(F):
    assert F.stats()["persist_aborts"] == 0


def _blocks_close(A, B, tol=TOL_FACTOR):
    err = np.max(np.abs(A - B)) / max(1e-300, np.max(np.abs(B)))
    assert err <= tol, (err, tol)
    return True


def _factor_tol(L):
    """Factor blocks against the twisted oracle: TOL_FACTOR, or 0.25 cond(S) eps (S = L L^T, the block it factors) where that is
    larger, as solve_tol does for solves.  The meeting block factors D_m - G_m G_m^T - H_m H_m^T, two rounded Schur
    corrections: two fp64 restatements of it (H_m by triangular solve, or by the explicit inverse as on the device) already
    differ by 6.5e-12 of max |L_m| on darcy256, cond(L_m) ~ 1e4; the reversed chain's blocks of burgers4096 sit at 1.3e-11."""
    return max(TOL_FACTOR, 0.25 * np.linalg.cond(L) ** 2 * EPS)


_SMALL = ["darcy32", "darcy64", "burgers64x8", "elliptic32", "rand"]


@pytest.fixture(scope="module", params=_SMALL)
def small(request, pkg):
    w = pkg.workloads.random_block_tridiagonal(9, 64, seed=4) if request.param == "rand" else pkg.workloads.make(request.param)
    F = _twisted(pkg, w)
    Fo = O.tridiagonal_cholesky(w.Q, w.n_blocks)
    Ft = TW.tridiagonal_cholesky(w.Q, w.n_blocks, F.meet)
    return w, F, Fo, Ft


def test_small_order_invariant(small, pkg):
    w, F, Fo, Ft = small
    assert F.order == "twisted" and 0 <= F.meet <= w.n_blocks - 1
    assert w.n_blocks < 3 or F.meet < w.n_blocks - 1
    tol = solve_tol(w)
    rng = np.random.default_rng(1)
    for k in (1, 16, 33, 64):
        B = w.rhs if k == 1 else rng.standard_normal((w.n, k))
        assert rel(pkg.ldiv(F, B), O.ldiv(Fo, B)) < tol, k
    assert abs(F.logdet() - O.logdet(Fo)) <= 1e-11 * abs(O.logdet(Fo)) + 1e-9
    vo = O.marginal_variances_exact(Fo)
    assert np.max(np.abs(F.marginal_var("exact") - vo) / vo) < _var_tol(w)
    _no_aborts(F)


def test_small_order_specific(small, pkg):
    w, F, Fo, Ft = small
    N, m = w.n_blocks, F.meet
    tol = solve_tol(w)
    rng = np.random.default_rng(2)
    B = rng.standard_normal((w.n, 3))
    assert rel(pkg.forward_solve(F, B), TW.forward_solve(Ft, B)) < tol
    assert rel(pkg.backward_solve(F, B), TW.backward_solve(Ft, B)) < tol
    for i in sorted({0, max(m - 1, 0), m, min(m + 1, N - 1), N - 1}):
        D = Ft.block("L", i)
        assert _blocks_close(F.get_block(0, i), D, _factor_tol(D)), ("L", i)
        # (the inverse against the oracle's block: its residual, which does not carry the block's condition number twice)
        assert np.max(np.abs(F.get_block(2, i) @ D - np.eye(D.shape[0]))) < max(1e-10, tol), ("LINV", i)
        if i < N - 1:
            assert _blocks_close(F.get_block(1, i), Ft.block("C", i)), ("C", i)
    assert np.allclose(np.tril(F.chos[N - 1], -1) if m < N - 1 else np.triu(F.chos[N - 1], 1), 0.0)
    Z = rng.standard_normal((w.n, 16))
    mu = pkg.ldiv(F, w.rhs)
    assert rel(F.sample(16, mean=mu, z=Z), TW.sample(Ft, mu, Z)) < tol
    _no_aborts(F)


def test_small_sampled_variances(small, pkg):
    w, F, Fo, Ft = small
    k, seed = 40, 17
    z = F.normals(k, seed=seed)
    X = TW.backward_solve(Ft, z)
    tol = 4.0 * solve_tol(w)
    Q = pkg.CsrMatrix(w.Q)
    assert rel(F.marginal_var("mc", k=k, seed=seed), O.marginal_variances_mc(X)) < tol
    assert rel(F.marginal_var("rbmc", k=k, seed=seed, Q=Q), O.marginal_variances_rbmc(w.Q, X)) < tol
    acc = np.zeros(w.n)
    F.var_accumulate(acc, "mc", 0, k, seed=seed)
    assert rel(acc / k, O.marginal_variances_mc(X)) < tol
    _no_aborts(F)


def test_meet_sweep_and_reference_bitwise(pkg):
    w = pkg.workloads.make("darcy32")
    N = w.n_blocks
    Fo = O.tridiagonal_cholesky(w.Q, N)
    mu_o, vo = O.ldiv(Fo, w.rhs), O.marginal_variances_exact(Fo)
    tol = solve_tol(w)
    R = pkg.tridiagonal_cholesky(w.Q, N)
    Z = np.random.default_rng(3).standard_normal((w.n, 8))
    for meet in (0, 1, None, N - 2, N - 1):
        F = _twisted(pkg, w, meet)
        m = F.meet
        assert meet is None or m == meet
        Ft = TW.tridiagonal_cholesky(w.Q, N, m)
        assert rel(pkg.ldiv(F, w.rhs), mu_o) < tol
        assert np.max(np.abs(F.marginal_var("exact") - vo) / vo) < _var_tol(w)
        assert rel(F.sample(8, z=Z), TW.sample(Ft, np.zeros(w.n), Z)) < tol
        if m == N - 1:                                   # the reference order, bitwise
            assert np.array_equal(pkg.ldiv(F, w.rhs), pkg.ldiv(R, w.rhs))
            assert np.array_equal(F.sample(8, z=Z), R.sample(8, z=Z))
            assert np.array_equal(F.sample(8, seed=5), R.sample(8, seed=5))
            assert np.array_equal(F.marginal_var("exact"), R.marginal_var("exact"))
            assert F.logdet() == R.logdet()
        _no_aborts(F)
        F.close()


def _check_full(pkg, w, first_last=8):
    N = w.n_blocks
    F = _twisted(pkg, w)
    m = F.meet
    assert 0 < m < N - 1
    Fo = O.tridiagonal_cholesky(w.Q, N)
    tol = solve_tol(w)
    assert rel(pkg.ldiv(F, w.rhs), O.ldiv(Fo, w.rhs)) < tol
    assert abs(F.logdet() - O.logdet(Fo)) <= 1e-11 * abs(O.logdet(Fo)) + 1e-9
    v = F.marginal_var("exact")
    vo = O.marginal_variances_exact(Fo)
    bs = w.n // N
    sel = np.r_[0:first_last * bs, m * bs:(m + 1) * bs, (N - first_last) * bs:N * bs]
    assert np.max(np.abs(v[sel] - vo[sel]) / vo[sel]) < _var_tol(w)
    Ft = TW.tridiagonal_cholesky(w.Q, N, m)
    for i in (m - 1, m, m + 1):
        D = Ft.block("L", i)
        assert _blocks_close(F.get_block(0, i), D, _factor_tol(D)), i
        assert _blocks_close(F.get_block(1, i), Ft.block("C", i)), i
    _no_aborts(F)
    return F


@pytest.mark.parametrize("name", ["burgers512x64", "darcy64", "darcy256"])
def test_full_size_configs(pkg, name):
    _check_full(pkg, pkg.workloads.make(name)).close()


def test_elliptic512_leading_slice(pkg):
    w = pkg.workloads.make("elliptic512")
    bs = w.n // w.n_blocks
    nb = 128
    Q = sp.csc_matrix(w.Q[:nb * bs, :nb * bs])
    Q.sort_indices()
    ws = pkg.workloads.Workload("elliptic512_slice", Q, np.asarray(w.rhs[:nb * bs]), nb, {})
    _check_full(pkg, ws).close()


def test_burgers4096_short_chain_256_column_panels(pkg):
    w = pkg.workloads.burgers(4096, 6)
    assert w.n // w.n_blocks == 4096
    F = _twisted(pkg, w)
    N, m = w.n_blocks, F.meet
    assert 0 < m < N - 1
    Fo = O.tridiagonal_cholesky(w.Q, N)
    tol = solve_tol(w)
    assert rel(pkg.ldiv(F, w.rhs), O.ldiv(Fo, w.rhs)) < tol
    assert abs(F.logdet() - O.logdet(Fo)) <= 1e-11 * abs(O.logdet(Fo)) + 1e-9
    Ft = TW.tridiagonal_cholesky(w.Q, N, m)
    for i in (m, m + 1):
        D = Ft.block("L", i)
        assert _blocks_close(F.get_block(0, i), D, _factor_tol(D)), i
    Z = np.random.default_rng(4).standard_normal((w.n, 2))
    assert rel(F.sample(2, z=Z), TW.sample(Ft, np.zeros(w.n), Z)) < tol
    _no_aborts(F)
    F.close()


def test_twisted_sample_covariance_matches_inverse(pkg):
    w = pkg.workloads.random_block_tridiagonal(6, 16, seed=21)
    F = _twisted(pkg, w)
    assert 0 < F.meet < w.n_blocks - 1
    k = 16384
    X = F.sample(k, seed=77)
    S = np.linalg.inv(w.Q.toarray())
    Chat = X @ X.T / k
    se = np.sqrt((np.outer(np.diag(S), np.diag(S)) + S * S) / k)
    assert np.max(np.abs(Chat - S) / se) < 6.0
    assert np.max(np.abs(X.mean(axis=1)) / np.sqrt(np.diag(S) / k)) < 6.0


def test_posterior_cabi_aliasing_and_torch(pkg):
    import torch
    w = pkg.workloads.make("darcy64")
    F = _twisted(pkg, w)
    n = w.n
    mean, samples = F.posterior(w.rhs, 20, seed=9, first_id=3)
    mu = pkg.ldiv(F, w.rhs)
    assert np.array_equal(mean, mu)
    assert np.array_equal(samples, F.sample(20, mean=mu, seed=9, first_id=3))
    # C ABI: ld = n + 7, mixed k, in place
    lib = pkg._cabi.load()
    ld = n + 7
    rng = np.random.default_rng(8)
    for k in (1, 5, 130):
        Bm = np.asfortranarray(rng.standard_normal((ld, k)))
        Y = np.zeros((ld, k), order="F")
        pkg._cabi.check(lib.gmrf_bt_solve(F._h, pkg._cabi.ptr(Bm), pkg._cabi.ptr(Y), k, ld, ld, 0))
        assert rel(Y[:n], pkg.ldiv(F, np.ascontiguousarray(Bm[:n]))) == 0.0
        Bi = Bm.copy(order="F")
        pkg._cabi.check(lib.gmrf_bt_solve(F._h, pkg._cabi.ptr(Bi), pkg._cabi.ptr(Bi), k, ld, ld, 0))
        assert np.array_equal(Bi[:n], Y[:n]) and np.array_equal(Bi[n:], Bm[n:])
        Z = np.asfortranarray(rng.standard_normal((ld, k)))
        S1 = np.zeros((ld, k), order="F")
        pkg._cabi.check(lib.gmrf_bt_sample(F._h, 1, 0, k, pkg._cabi.ptr(mu), pkg._cabi.ptr(Z), pkg._cabi.ptr(S1), ld))
        pkg._cabi.check(lib.gmrf_bt_sample(F._h, 1, 0, k, pkg._cabi.ptr(mu), pkg._cabi.ptr(Z), pkg._cabi.ptr(Z), ld))
        assert np.array_equal(S1[:n], Z[:n])
    # torch device I/O
    b = torch.from_numpy(w.rhs).cuda()
    mu_d = pkg.ldiv(F, b)
    assert mu_d.is_cuda and np.array_equal(mu_d.cpu().numpy(), mu)
    X = F.sample(16, mean=mu_d, seed=9, like=b)
    assert X.is_cuda and np.array_equal(X.cpu().numpy(), F.sample(16, mean=mu, seed=9))
    out = torch.empty(n, dtype=torch.float64, device="cuda")
    F.marginal_var("exact", out=out)
    assert np.array_equal(out.cpu().numpy(), F.marginal_var("exact"))
    _no_aborts(F)
    F.close()


def test_default_handle_unchanged_by_a_twisted_one(pkg):
    w = pkg.workloads.make("darcy64")
    R = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
    before = (pkg.ldiv(R, w.rhs), R.sample(8, seed=4), R.marginal_var("exact"), R.logdet())
    F = _twisted(pkg, w)
    pkg.ldiv(F, w.rhs); F.sample(8, seed=4); F.marginal_var("exact")
    F.close()
    after = (pkg.ldiv(R, w.rhs), R.sample(8, seed=4), R.marginal_var("exact"), R.logdet())
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


def test_errors_and_refused_calls(pkg):
    w = pkg.workloads.make("darcy32")
    N = w.n_blocks
    lib = pkg._cabi.load()
    F = pkg.TridiagonalCholeskyFactor()
    with pytest.raises(pkg.GmrfError) as e:
        pkg._cabi.check(lib.gmrf_bt_set_order(F._h, 7, -1))
    assert e.value.status == pkg._cabi.ERR_BAD_SHAPE
    F.set_order("twisted", N)                         # meet outside [0, N-1]: at factor time
    with pytest.raises(pkg.GmrfError) as e:
        F.factor(w.Q, N)
    assert e.value.status == pkg._cabi.ERR_BAD_SHAPE
    F.set_order("twisted", 2)
    F.factor(w.Q, N)
    assert F.meet == 2
    with pytest.raises(pkg.GmrfError) as e:
        F.set_batch(2)
    assert e.value.status == pkg._cabi.ERR_BAD_SHAPE and "twisted" in str(e.value)
    refused = [
        lambda: F.export_factor(),
        lambda: F.factor_blocks([sp.identity(4)], []),
        lambda: F.get_layout(),
        lambda: F.factor_buffer(0),
        lambda: F.packed_size(0, 1),
        lambda: F.set_keep_l(False),
        lambda: F.adopt_shape(w.n, N),
        lambda: pkg._cabi.check(lib.gmrf_bt_factor_begin_csc(F._h, 0, 0, None, None, None, 0)),
        lambda: pkg._cabi.check(lib.gmrf_bt_factor_end(F._h, None)),
        lambda: pkg._cabi.check(lib.gmrf_bt_marginal_var_batch(F._h, 2, 4, 0, None, None, pkg._cabi.ptr(np.zeros(w.n)))),
    ]
    for call in refused:
        with pytest.raises(pkg.GmrfError) as e:
            call()
        assert e.value.status == pkg._cabi.ERR_BAD_SHAPE and "twisted" in str(e.value)
    F.set_order("twisted", 2)                         # drops the factor
    with pytest.raises(pkg.GmrfError) as e:
        pkg.ldiv(F, w.rhs)
    assert e.value.status == pkg._cabi.ERR_NO_FACTOR
    F.close()
    # NOT_SPD: the failing block in original 1-based numbering, in the bottom half and in the meeting block
    Qb = w.Q.tolil()
    bs = w.n // N
    j = (N - 2) * bs + 3                               # a diagonal entry of block N-2 (bottom half for meet = 2)
    Qb[j, j] = -1e6
    F = pkg.TridiagonalCholeskyFactor(order="twisted", meet=2)
    with pytest.raises(pkg.NotPositiveDefinite) as e:
        F.factor(sp.csc_matrix(Qb), N)
    assert e.value.info == N - 1
    Qm = w.Q.tolil()
    j = 2 * bs + 5
    Qm[j, j] = -1e6
    F.set_order("twisted", 2)
    with pytest.raises(pkg.NotPositiveDefinite) as e:
        F.factor(sp.csc_matrix(Qm), N)
    assert e.value.info == 3
    F.close()

