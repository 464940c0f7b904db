"""The fused posterior's last backward products write the caller's mean and samples themselves (gemm_f64_dma DOUT) instead of a
pass of its own over the result panel: samples bitwise gmrf_bt_sample's around the fused mean, the mean against gmrf_bt_solve as
tests/test_gpu_fused_posterior.py composes them, leading dimensions beyond n, blocks narrower than their padding, sample counts
below their padding, and the routes that do not fuse.

The fused pass needs the samples' sweep on the GEMM: batch * (padded block / 64) * (padded k / 64) >= 128 tiles (posterior_fused_ok).
Blocks of 256 reach that at a batch of 32 for k = 64 and of 16 for k = 128; a batch of 8 stays on the two calls for either k and is
checked as that."""
import numpy as np
import pytest

from tests.test_gpu_grouped_gemm import chain
from tests.test_gpu_parity import rel

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e300


def _fused(F):
    """Did the last gmrf_bt_posterior take the fused pass?  (it books the whole call in solve_ms, sample_ms = 0)"""
    return F.stats()["sample_ms"] == 0.0


_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    """The shared handles live as long as this module: closed after its last test, so that their persistent claims on the chip
    are free again for the modules that run later."""
    yield
    for F, _ in _CACHE.values():
        F.close()
    _CACHE.clear()


def _batch(pkg, bs, nb, B, corner=0):
    """One factored handle per shape (shared, never changed by a test)."""
    import torch
    key = (bs, nb, B, corner)
    if key not in _CACHE:
        Q = chain(bs, nb, seed=bs + nb, corner=corner)
        vals = np.stack([Q.data * (1.0 + 0.05 * p) for p in range(B)])
        F = pkg.TridiagonalCholeskyFactor(batch=B).factor(Q, nb, values=vals)
        rng = np.random.default_rng(B)
        b = torch.from_numpy(rng.standard_normal((B, Q.shape[0]))).cuda()
        _CACHE[key] = (F, b)
    return _CACHE[key]


def _posterior_ld(pkg, lib, F, b, k, ld, seed, first):
    """gmrf_bt_posterior into sentinel-filled arrays: samples with leading dimension ld and a guard behind both outputs."""
    import torch
    B, n = b.shape
    guard = 4096
    mean_buf = torch.full((B * n + guard,), SENTINEL, dtype=torch.float64, device=b.device)
    smp_buf = torch.full((B * k * ld + guard,), SENTINEL, dtype=torch.float64, device=b.device)
    pkg._cabi.check(lib.gmrf_bt_posterior(F._h, pkg._cabi.ptr(b), seed, first, k, pkg._cabi.ptr(mean_buf), pkg._cabi.ptr(smp_buf), ld))
    assert bool((mean_buf[B * n:] == SENTINEL).all()) and bool((smp_buf[B * k * ld:] == SENTINEL).all())
    X = smp_buf[:B * k * ld].view(B, k, ld)
    assert bool((X[:, :, n:] == SENTINEL).all())
    return mean_buf[:B * n].view(B, n).clone(), X[:, :, :n].clone()


# bs, nb, batch, k, corner, fused
CASES = [(256, 3, 32, 64, 0, True), (256, 3, 16, 128, 0, True), (256, 3, 8, 64, 0, False), (256, 3, 8, 128, 0, False),
         (200, 3, 32, 64, 0, True),       # blocks of 200 in a padding of 256: not a multiple of 64
         (200, 3, 32, 50, 0, True),       # 50 samples in 64 panel rows
         (200, 3, 16, 100, 0, False),     # 100 samples in 112 panel rows, not a multiple of 64: the two calls
         (512, 3, 16, 64, 128, True)]     # coupling blocks in a corner window (the split block inverses where the plan takes them)


@pytest.mark.parametrize("bs,nb,B,k,corner,fused", CASES)
def test_direct_output_against_solve_and_sample(pkg, lib, bs, nb, B, k, corner, fused):
    F, b = _batch(pkg, bs, nb, B, corner)
    n = bs * nb
    seed, first = 11, 500
    mu_u = F.solve_batch(b[:, None, :])[:, 0, :]
    for ld in (n, n + 3, n + 64):
        mu_f, X_f = _posterior_ld(pkg, lib, F, b, k, ld, seed, first)
        assert _fused(F) == fused
        if fused:
            assert rel(mu_f.cpu().numpy(), mu_u.cpu().numpy()) < 1e-12
        else:
            assert bool((mu_f == mu_u).all())
        # the samples are gmrf_bt_sample's around that mean: the same bits
        X_s = F.sample_batch(k, mean=mu_f, seed=seed, first_id=first, like=b)
        assert bool((X_s == X_f).all())
    # the wrapper (ld = n, its own arrays) gives the same bits as the sentinel-filled call
    mu_w, X_w = F.posterior_batch(b, k, seed=seed, first_id=first)
    assert bool((mu_w == mu_f).all()) and bool((X_w == X_f).all())


def test_other_output_arrays_on_the_same_captured_sweep(pkg, lib):
    """The sweep's captured graph holds no pointer of a call: a second call with other arrays, another ld and another k under the
    same padded k writes those arrays (and nothing beyond them: the sentinels of _posterior_ld)."""
    F, b = _batch(pkg, 200, 3, 32)
    n = 600
    mu1, X1 = _posterior_ld(pkg, lib, F, b, 64, n, 3, 0)
    mu2, X2 = _posterior_ld(pkg, lib, F, b, 50, n + 8, 3, 0)
    assert _fused(F)
    assert bool((mu2 == mu1).all()) and bool((X2[0] == X1[0, :50]).all())      # (problem 0 draws the same sample ids)
    X_s = F.sample_batch(50, mean=mu2, seed=3, first_id=0, like=b)
    assert bool((X_s == X2).all())


def test_k17_keeps_the_two_calls(pkg, lib):
    F, b = _batch(pkg, 256, 3, 32)
    k, seed, first = 17, 5, 40
    mu_f, X_f = _posterior_ld(pkg, lib, F, b, k, 768 + 5, seed, first)
    assert not _fused(F)
    assert bool((mu_f == F.solve_batch(b[:, None, :])[:, 0, :]).all())
    assert bool((F.sample_batch(k, mean=mu_f, seed=seed, first_id=first, like=b) == X_f).all())
