"""GPU tests of the selected inverse on a pattern (gmrf_bt_selinv, TridiagonalCholeskyFactor.selected_inverse) and of
tr(Q^-1 dQ) (gmrf_bt_trace_inv): against the dense inverse, against the NumPy recurrence of tests/selinv_oracle.py at full
size, against the exact variances, sub-patterns, batches, the log-determinant's derivative, and the errors of the call.
Entry errors are measured on the correlation scale |Sigma_hat_rc - Sigma_rc| / sqrt(Sigma_rr Sigma_cc)."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import bt_oracle as O
from tests import selinv_oracle as SI
from tests.test_gpu_parity import EPS, solve_tol

pytestmark = pytest.mark.gpu


def _tol(w):
    return max(1e-10, 4.0 * solve_tol(w))


def _rows(S):
    return np.repeat(np.arange(S.shape[0]), np.diff(S.indptr))


def _csr(Q):
    S = sp.csr_matrix(Q)
    S.sort_indices()
    return S


def _dense_check(pkg, w):
    S = _csr(w.Q)
    F = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
    got = F.selected_inverse(pkg.CsrMatrix(S))
    assert isinstance(got, sp.csr_matrix)
    assert np.array_equal(got.indptr, S.indptr) and np.array_equal(got.indices, S.indices)
    Sigma = np.linalg.inv(w.Q.toarray())
    d = np.sqrt(np.diag(Sigma))
    r, c = _rows(S), S.indices
    err = SI.entry_error(got.data, Sigma[r, c], d[r] * d[c])
    assert err <= _tol(w), (w.name, err, _tol(w))
    return F, S, got


@pytest.mark.parametrize("name", ["darcy64", "rand100", "rand256"])
def test_against_dense_inverse(pkg, name):
    if name == "darcy64":
        w = pkg.workloads.make("darcy64")
    else:
        bs = int(name[4:])
        w = pkg.workloads.random_block_tridiagonal(6 if bs == 100 else 4, bs, seed=5)
    _dense_check(pkg, w)


def _oracle_check(pkg, w, Q, n_blocks, last_blocks=0):
    S = _csr(Q)
    F = pkg.tridiagonal_cholesky(Q, n_blocks)
    got = F.selected_inverse(pkg.CsrMatrix(S)).data
    Fo = O.tridiagonal_cholesky(Q, n_blocks)
    want, mask, scale = SI.pattern_values(Fo, S, last_blocks)
    assert mask.sum() > 0
    err = SI.entry_error(got, want, scale, mask)
    tol = max(1e-9, 0.01 * w.meta["cond"] * EPS)
    print("selinv against the oracle:", w.name, "entries", int(mask.sum()), "err", err, "tol", tol)
    assert err <= tol, (w.name, err, tol)


def test_against_oracle_burgers512x64(pkg):
    w = pkg.workloads.make("burgers512x64")
    solve_tol(w)                                   # fills meta["cond"]
    _oracle_check(pkg, w, w.Q, w.n_blocks)


def test_against_oracle_darcy256(pkg):
    w = pkg.workloads.make("darcy256")
    w.meta.setdefault("cond", 3.4e9)               # as test_config_darcy256_against_oracle (eigsh at n = 65536 takes minutes)
    _oracle_check(pkg, w, w.Q, w.n_blocks)


def test_against_oracle_elliptic512_leading_blocks(pkg):
    """The leading 128 of elliptic512's 256 blocks (as test_measured_path_elliptic512_batch8_against_oracle slices it): the
    entries of the last two diagonal blocks and of the coupling block between them."""
    w = pkg.workloads.make("elliptic512")
    w.meta.setdefault("cond", 4.04e9)
    nbk = 128
    ns = nbk * w.block_size
    Qs = w.Q.tocsr()[:ns, :ns].tocsc()
    Qs.sort_indices()
    _oracle_check(pkg, w, Qs, nbk, last_blocks=2)


@pytest.fixture(scope="module")
def darcy64(pkg):
    w = pkg.workloads.make("darcy64")
    S = _csr(w.Q)
    F = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
    return w, S, pkg.CsrMatrix(S), F


def test_diagonal_equals_exact_variances(pkg, darcy64):
    w, S, Sd, F = darcy64
    got = F.selected_inverse(Sd)
    v = F.marginal_var("exact")
    assert np.max(np.abs(got.diagonal() - v) / v) <= 1e-11
    for name, N in (("burgers64x8", None), ("rand", 5)):
        w2 = pkg.workloads.make(name) if N is None else pkg.workloads.random_block_tridiagonal(N, 100, seed=2)
        F2 = pkg.tridiagonal_cholesky(w2.Q, w2.n_blocks)
        d = F2.selected_inverse(pkg.CsrMatrix(_csr(w2.Q))).diagonal()
        v2 = F2.marginal_var("exact")
        assert np.max(np.abs(d - v2) / v2) <= 1e-11, name


def test_sub_patterns_give_the_same_values(pkg, darcy64):
    w, S, Sd, F = darcy64
    full = F.selected_inverse(Sd)
    bs = w.block_size
    r = _rows(S)
    keep = (r // bs) == (S.indices // bs)                     # the diagonal blocks D_i only
    D = sp.csr_matrix((S.data[keep], (r[keep], S.indices[keep])), shape=S.shape)
    L = _csr(sp.tril(S))
    for P in (D, L):
        P = _csr(P)
        got = F.selected_inverse(pkg.CsrMatrix(P))
        pr = _rows(P)
        want = np.asarray(full[pr, P.indices]).ravel()
        assert np.array_equal(got.data, want)


def test_batch_of_four_against_single_handles(pkg, darcy64):
    import torch
    w, S, Sd, _ = darcy64
    B = 4
    Qc = sp.csc_matrix(w.Q)
    Qc.sort_indices()
    dg = Qc.diagonal()
    mats = [(Qc + sp.diags(0.05 * p * dg)).tocsc() for p in range(B)]
    for M in mats:
        M.sort_indices()
        assert np.array_equal(M.indptr, Qc.indptr) and np.array_equal(M.indices, Qc.indices)
    F = pkg.TridiagonalCholeskyFactor(batch=B)
    F.factor(Qc, w.n_blocks, values=np.stack([M.data for M in mats]))
    got = F.selected_inverse(Sd)
    assert got.shape == (B, S.nnz)
    r, c = _rows(S), S.indices
    for p, M in enumerate(mats):
        Fp = pkg.tridiagonal_cholesky(M, w.n_blocks)
        want = Fp.selected_inverse(Sd)
        d = np.sqrt(want.diagonal())
        assert SI.entry_error(got[p], want.data, d[r] * d[c]) <= _tol(w), p
    dev = torch.empty((B, S.nnz), dtype=torch.float64, device="cuda")
    assert F.selected_inverse(Sd, out=dev) is dev
    assert np.array_equal(dev.cpu().numpy(), got)
    host = np.empty((B, S.nnz))
    assert F.selected_inverse(Sd, out=host) is host
    assert np.array_equal(host, got)
    with pytest.raises(ValueError):
        F.selected_inverse(Sd, out=np.empty(S.nnz))
    # trace_inv of a batch: (batch, m, nnz) -> (batch, m), against the values it is a dot product of
    dv = np.random.default_rng(3).standard_normal((B, 2, S.nnz))
    tr = F.trace_inv(Sd, dv)
    assert tr.shape == (B, 2)
    assert np.max(np.abs(tr - np.einsum("pe,pje->pj", got, dv))) <= 1e-12 * np.max(np.abs(got)) * S.nnz


def _trace_q(pkg, w):
    S = _csr(w.Q)
    Sd = pkg.CsrMatrix(S)
    F = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
    return S, Sd, F


@pytest.mark.parametrize("case", ["laplace", "ar1", "rand"])
def test_trace_inv_of_q_and_identity(pkg, case):
    w = {"laplace": lambda: pkg.workloads.laplace_kappa_grid(70, 12, kappa2=0.5),
         "ar1": lambda: pkg.workloads.ar1_chain_kron_identity(8, 96, phi=0.6),
         "rand": lambda: pkg.workloads.random_block_tridiagonal(5, 100, seed=9)}[case]()
    S, Sd, F = _trace_q(pkg, w)
    eye = (_rows(S) == S.indices).astype(np.float64)
    tr = F.trace_inv(Sd, np.stack([S.data, eye]))
    assert tr.shape == (2,)
    assert abs(tr[0] - w.n) <= 1e-9 * w.n, (tr[0], w.n)
    v = F.marginal_var("exact")
    assert abs(tr[1] - v.sum()) <= 1e-11 * abs(v.sum())
    tr2 = F.trace_inv(Sd, np.stack([S.data, eye]))
    assert np.array_equal(tr, tr2)


def test_trace_inv_is_the_logdet_derivative_matern(pkg):
    """d logdet Q / d kappa on the alpha = 2 Matern prior of workloads.matern_precision_2d (64 x 64 nodes, tau held fixed):
    Q = tau^2 K C^-1 K, K = kappa^2 C + G, dQ/dkappa = tau^2 (dK C^-1 K + K C^-1 dK), dK = 2 kappa C; against the central
    difference of the GPU logdet at kappa (1 +- 1e-4)."""
    import torch
    nx = 64
    lumped, G, _, _ = pkg.workloads.p1_unit_square(nx, nx)
    C = sp.diags(lumped)
    Ci = sp.diags(1.0 / lumped)
    kappa = math.sqrt(8.0) / 0.2
    tau2 = 1.0 / (4.0 * math.pi * kappa ** 2)          # alpha = 2 (nu = 1) at the base kappa, then held fixed
    n_blocks = nx // 4

    def Q_of(k):
        K = (k * k) * C + G
        Q = (tau2 * (K @ Ci @ K)).tocsr()
        return _csr((Q + Q.T) * 0.5)

    Q = Q_of(kappa)
    K = (kappa * kappa) * C + G
    dK = (2.0 * kappa) * C
    dQ = (tau2 * (dK @ Ci @ K + K @ Ci @ dK)).tocsr()
    dQ = (dQ + dQ.T) * 0.5
    dvals = np.asarray(dQ[_rows(Q), Q.indices]).ravel()
    Sd = pkg.CsrMatrix(Q)
    F = pkg.tridiagonal_cholesky(Q, n_blocks)
    g = F.trace_inv(Sd, dvals[None, :])[0]
    h = 1e-4
    lp = pkg.tridiagonal_cholesky(Q_of(kappa * (1 + h)), n_blocks).logdet()
    lm = pkg.tridiagonal_cholesky(Q_of(kappa * (1 - h)), n_blocks).logdet()
    fd = (lp - lm) / (2.0 * kappa * h)
    assert abs(g - fd) <= 1e-6 * abs(fd), (g, fd)
    # device operands give the same bits
    dv_t = torch.from_numpy(dvals[None, :].copy()).cuda()
    g_t = F.trace_inv(Sd, dv_t)
    assert g_t.is_cuda and g_t.cpu().numpy()[0] == g


def test_other_calls_unchanged_around_selected_inverse(pkg, darcy64):
    w, S, Sd, _ = darcy64
    F = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)

    def run():
        return (F.marginal_var("exact"), pkg.ldiv(F, w.rhs), F.sample(8, seed=1234), F.logdet())

    before = run()
    F.selected_inverse(Sd)
    F.trace_inv(Sd, S.data[None, :])
    after = run()
    for a, b in zip(before, after):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def _status(excinfo):
    return excinfo.value.status


def test_errors(pkg, darcy64):
    w, S, Sd, F = darcy64
    cabi = pkg._cabi
    bs, n = w.block_size, w.n
    # two blocks apart
    E = S.tolil(copy=True)
    E[0, 2 * bs] = 1.0
    E[2 * bs, 0] = 1.0
    with pytest.raises(cabi.GmrfError) as ei:
        F.selected_inverse(pkg.CsrMatrix(_csr(E)))
    assert _status(ei) == cabi.ERR_BAD_SHAPE and "(0, " in str(ei.value)
    # a coupling entry whose row in the later block is >= rmax
    rmax = int(F.get_layout()[1])
    assert rmax < bs
    E = S.tolil(copy=True)
    E[bs + bs - 1, 0] = 1.0
    with pytest.raises(cabi.GmrfError) as ei:
        F.selected_inverse(pkg.CsrMatrix(_csr(E)))
    assert _status(ei) == cabi.ERR_BAD_SHAPE and "rmax" in str(ei.value)
    with pytest.raises(cabi.GmrfError) as ei:
        F.trace_inv(pkg.CsrMatrix(_csr(E)), np.ones((1, E.nnz)))
    assert _status(ei) == cabi.ERR_BAD_SHAPE
    # the handle still serves the valid pattern
    assert np.all(np.isfinite(F.selected_inverse(Sd).data))
    # a twisted handle
    T = pkg.TridiagonalCholeskyFactor(order="twisted")
    T.factor(w.Q, w.n_blocks)
    for call in (lambda: T.selected_inverse(Sd), lambda: T.trace_inv(Sd, S.data[None, :])):
        with pytest.raises(cabi.GmrfError) as ei:
            call()
        assert _status(ei) == cabi.ERR_BAD_SHAPE and "twisted" in str(ei.value)
    # before a factor
    G = pkg.TridiagonalCholeskyFactor()
    for call in (lambda: G.selected_inverse(Sd), lambda: G.trace_inv(Sd, S.data[None, :])):
        with pytest.raises(cabi.GmrfError) as ei:
            call()
        assert _status(ei) == cabi.ERR_NO_FACTOR


def test_conditioned_gmrf_selected_inverse(pkg):
    w = pkg.workloads.laplace_kappa_grid(64, 8, kappa2=0.5)
    n = w.n
    obs = np.arange(0, n, 7)
    A = sp.csr_matrix((np.ones(obs.size), (np.arange(obs.size), obs)), shape=(obs.size, n))
    y = np.random.default_rng(0).standard_normal(obs.size)
    post = pkg.condition_on_observations(w.Q, None, A, 4.0, y, w.n_blocks)
    Sig = post.selected_inverse()
    P = _csr(post.precision_matrix())
    assert np.array_equal(Sig.indptr, P.indptr) and np.array_equal(Sig.indices, P.indices)
    v = post.var("exact")
    assert np.max(np.abs(Sig.diagonal() - v) / v) <= 1e-11
    Sigma = np.linalg.inv(P.toarray())
    d = np.sqrt(np.diag(Sigma))
    r = _rows(P)
    assert SI.entry_error(Sig.data, Sigma[r, P.indices], d[r] * d[P.indices]) <= 1e-10
