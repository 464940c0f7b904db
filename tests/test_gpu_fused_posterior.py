"""The fused posterior of a batch (gmrf_bt_posterior, B > 1): the mean's backward sweep carried as the tail row of the samples'
GEMMs (gemm_f64_dma TAIL) -- against the two-call route (set_eager bit 18: gmrf_bt_solve + gmrf_bt_sample), the oracle, and
the tail-row GEMM against the 64-row kernel."""
import numpy as np
import pytest
import scipy.sparse as sp

import __graft_entry__
from oracle import bt_oracle as O
from tests.test_gpu_parity import rel, solve_tol

pytestmark = pytest.mark.gpu

Switch = __graft_entry__.load_package().Switch
TAIL = 65536                 # gmrf_test_gemm: the 64 x 64 LDS-DMA kernel with the tail row


def _leading(w, nb):
    """The leading nb blocks of a workload (a principal submatrix: SPD, block tridiagonal)."""
    m = nb * w.block_size
    Q = sp.csc_matrix(w.Q[:m, :m])
    Q.sort_indices()
    return Q, np.ascontiguousarray(w.rhs[:m]), nb


def _batch(pkg, Q, rhs, nb, B):
    import torch
    vals = np.stack([Q.data * (1.0 + 0.05 * p) for p in range(B)])
    F = pkg.TridiagonalCholeskyFactor(batch=B).factor(Q, nb, values=vals)
    b = torch.from_numpy(np.stack([rhs * (1.0 + 0.5 * p) for p in range(B)])).cuda()
    return F, vals, b


def _fused(F):
    """Did the last gmrf_bt_posterior take the fused pass?  (it books the whole call in solve_ms, sample_ms = 0)"""
    return F.stats()["sample_ms"] == 0.0


CASES = {"darcy256_leading8": ("darcy256", 8, 12), "burgers512x64": ("burgers512x64", None, 16)}


@pytest.fixture(scope="module", params=list(CASES))
def batch_case(request, pkg):
    name, nb, B = CASES[request.param]
    w = pkg.workloads.make(name)
    if name == "darcy256":
        w.meta.setdefault("cond", 3.4e9)       # the whole posterior's (a principal submatrix's is not larger)
    Q, rhs, nb = _leading(w, nb) if nb else (w.Q, w.rhs, w.n_blocks)
    F, vals, b = _batch(pkg, Q, rhs, nb, B)
    return w, Q, rhs, nb, B, F, vals, b


def test_fused_posterior_against_two_calls_and_oracle(pkg, batch_case):
    w, Q, rhs, nb, B, F, vals, b = batch_case
    k, seed, first = 64, 77, 1000
    mu_f, X_f = F.posterior_batch(b, k, seed=seed, first_id=first)
    assert _fused(F)
    assert mu_f.shape == (B, Q.shape[0]) and X_f.shape == (B, k, Q.shape[0])
    # the samples' L^-T z rows are bitwise gmrf_bt_sample's: its samples around the fused mean are the same bits
    X_s = F.sample_batch(k, mean=mu_f, seed=seed, first_id=first, like=b)
    assert bool((X_s == X_f).all())
    # the two-call route (eager bit 18): the mean to rounding, the samples around their own mean
    F.set_eager(Switch.TWO_CALL_POSTERIOR)
    try:
        mu_u, X_u = F.posterior_batch(b, k, seed=seed, first_id=first)
        assert not _fused(F)
    finally:
        F.set_eager(0)
    tol = solve_tol(w)
    mu_f_h, mu_u_h = mu_f.cpu().numpy(), mu_u.cpu().numpy()
    X_f_h, X_u_h = X_f.cpu().numpy(), X_u.cpu().numpy()
    for p in range(B):
        assert rel(mu_f_h[p], mu_u_h[p]) < 1e-12
        assert rel(X_f_h[p], X_u_h[p]) < 1e-12
    assert bool((F.solve_batch(b[:, None, :])[:, 0, :] == mu_u).all())
    # the oracle, first and last problem
    Z = F.normals_batch(k, seed=seed, first_id=first)
    for p in (0, B - 1):
        Qp = Q.copy(); Qp.data = vals[p]
        Fo = O.tridiagonal_cholesky(Qp, nb)
        mu_o = O.ldiv(Fo, rhs * (1.0 + 0.5 * p))
        assert rel(mu_f_h[p], mu_o) < tol
        assert rel(X_f_h[p].T, O.sample(Fo, mu_o, Z[p].T)) < tol


@pytest.mark.parametrize("k", [1, 17, 64, 65, 128, 130])
def test_fused_posterior_sample_counts(pkg, k):
    """k that pads to 1 / 32 / 80 rows stays on the two calls (bitwise), 64 / 128 fuse (one and two 64-row tiles with the tail on
    the second), 130 > 128 goes in chunks through the engine (two calls)."""
    import torch
    w = pkg.workloads.make("burgers512x64")
    B = 16
    F, vals, b = _batch(pkg, w.Q, w.rhs, w.n_blocks, B)
    seed, first = 5, 40
    if k > 128:
        import importlib
        post = importlib.import_module(pkg.__name__ + ".posterior")
        with torch.cuda.stream(torch.cuda.Stream()):       # (the engine keeps the thread's current stream)
            e = post.HipEngine(pkg, w, batch=B, values=vals, rhs=b.cpu().numpy())
            e.prepare(is_root=True, shared_storage=False)
            mu, X = e.posterior(k, seed, first)
            mu2 = e.mean()
            assert bool((mu == mu2).all()) and X.shape == (B, k, w.n)
            assert bool((X == e.sample(k, mu2, seed, first)).all())
            e.synchronize()
        return
    mu_f, X_f = F.posterior_batch(b, k, seed=seed, first_id=first)
    fused = k in (64, 128)
    assert _fused(F) == fused
    mu_u = F.solve_batch(b[:, None, :])[:, 0, :]
    if fused:
        assert rel(mu_f.cpu().numpy(), mu_u.cpu().numpy()) < 1e-12
    else:
        assert bool((mu_f == mu_u).all())
    X_s = F.sample_batch(k, mean=mu_f, seed=seed, first_id=first, like=b)
    assert bool((X_s == X_f).all())
    assert torch.isfinite(X_f).all()


def test_fused_posterior_aliased_input_takes_two_calls(pkg, lib):
    """b IS the mean's output: the fused pass would overwrite it while the sweeps still read it -- the two-call route runs, and
    gives what the same call on separate buffers gives through the two calls."""
    import torch
    w = pkg.workloads.make("burgers512x64")
    B, k = 16, 64
    F, vals, b = _batch(pkg, w.Q, w.rhs, w.n_blocks, B)
    F.set_eager(Switch.TWO_CALL_POSTERIOR)
    mu_ref, X_ref = F.posterior_batch(b, k, seed=3, first_id=0)
    F.set_eager(0)
    bm = b.clone()
    X = torch.empty((B, k, w.n), dtype=torch.float64, device=b.device)
    pkg._cabi.check(lib.gmrf_bt_posterior(F._h, pkg._cabi.ptr(bm), 3, 0, k, pkg._cabi.ptr(bm), pkg._cabi.ptr(X), w.n))
    assert not _fused(F)
    assert bool((bm == mu_ref).all()) and bool((X == X_ref).all())
    # the same call without the overlap fuses
    mu_f, X_f = F.posterior_batch(b, k, seed=3, first_id=0)
    assert _fused(F)
    assert rel(mu_f.cpu().numpy(), mu_ref.cpu().numpy()) < 1e-12


@pytest.mark.parametrize("M,N,K,tri,beta", [(64, 64, 64, 0, 0.0), (64, 256, 768, 0, 1.0), (128, 192, 256, 4, 0.0),
                                            (64, 1024, 1024, 4, 0.0), (128, 512, 512, 0, -1.0)])
def test_tail_row_gemm_against_64_row_kernel(lib, pkg, M, N, K, tri, beta):
    """C = alpha A B + beta C with B stored [k][n]: rows 0 .. M-1 bitwise the 64 x 64 LDS-DMA kernel's, row M (the tail) against a
    float64 NumPy reference."""
    rng = np.random.default_rng(M + N + K + tri)
    A = rng.standard_normal((M + 1, K))
    Bm = rng.standard_normal((K, N))
    if tri & 4:
        Bm = np.tril(Bm)
    C0 = rng.standard_normal((M + 1, N))
    alpha = -1.0 if beta else 1.0
    out_t = C0.copy()
    pkg._cabi.check(lib.gmrf_test_gemm(0, M, N, K, 0, 0, tri | TAIL, 0, alpha, pkg._cabi.ptr(A), K, pkg._cabi.ptr(Bm), N, beta,
                                       pkg._cabi.ptr(out_t), N))
    out_m = C0[:M].copy()
    Am = np.ascontiguousarray(A[:M])
    pkg._cabi.check(lib.gmrf_test_gemm(0, M, N, K, 0, 0, tri | 8192, 0, alpha, pkg._cabi.ptr(Am), K, pkg._cabi.ptr(Bm), N, beta,
                                       pkg._cabi.ptr(out_m), N))
    assert np.array_equal(out_t[:M], out_m)
    ref = alpha * (A[M] @ Bm) + beta * C0[M]
    scale = np.abs(A[M]) @ np.abs(Bm) + abs(beta) * np.abs(C0[M])
    assert np.max(np.abs(out_t[M] - ref) / scale) < 1e-15 * K
    assert np.max(np.abs(out_m - (alpha * (A[:M] @ Bm) + beta * C0[:M]))) < 1e-12 * K
