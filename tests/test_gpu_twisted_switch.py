"""GPU tests of the twisted order on a handle with a history: switched from a reference-order factor (persistent launches,
other shapes), and re-factored with new values from the host and from the device."""
import gc

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import bt_oracle as O
from tests.test_gpu_parity import rel, solve_tol
from tests.test_gpu_twisted import _no_aborts, _twisted

pytestmark = pytest.mark.gpu


def _shifted(Q, frac):
    """Q with its diagonal raised by frac * mean |diag| (same pattern: CSC sorted as factor() takes it)."""
    A = sp.csc_matrix(Q, copy=True)
    A.sort_indices()
    cols = np.repeat(np.arange(A.shape[1]), np.diff(A.indptr))
    A.data = A.data.copy()
    A.data[A.indices == cols] += frac * np.abs(A.diagonal()).mean()
    return A


def _check_mean_logdet(pkg, F, Q, rhs, N, tol):
    Fo = O.tridiagonal_cholesky(Q, N)
    mu = pkg.ldiv(F, rhs)
    assert rel(mu, O.ldiv(Fo, rhs)) < tol
    assert abs(F.logdet() - O.logdet(Fo)) <= 1e-11 * abs(O.logdet(Fo)) + 1e-9
    return mu


def test_switch_from_a_persistent_reference_factor(pkg):
    """A handle factored in the reference order (blocks of 512: persistent sweeps, a claim on the whole chip) is switched to the
    twisted order: the halves get their persistent claims and the posterior runs on the twisted factor -- with the same shape
    and with a new one (the handle's own buffers of the old shape are gone)."""
    import torch
    gc.collect()                                     # (handles of earlier tests give their claims back)
    w = pkg.workloads.make("burgers512x64")
    N = w.n_blocks
    F = pkg.TridiagonalCholeskyFactor()
    F.factor(w.Q, N)
    assert F.stats()["persist_cus"] > 0
    b = torch.from_numpy(w.rhs).cuda()
    F.posterior(b, 16, seed=2)
    assert F.stats()["sweep_persist"] == 1
    v = pkg.workloads.burgers(512, 32)
    for Q, rhs, nb in ((_shifted(w.Q, 0.5), w.rhs, N), (v.Q, v.rhs, v.n_blocks)):
        F.set_order("twisted")
        F.factor(Q, nb)
        assert 0 < F.meet < nb - 1
        assert F.half_stats(0)["persist_cus"] > 0 and F.half_stats(1)["persist_cus"] > 0
        # (raising the diagonal of an SPD matrix does not raise its condition number: the workload's own bound holds)
        tol = solve_tol(w) if nb == N else solve_tol(v)
        bd = torch.from_numpy(rhs).cuda()
        mean, samples = F.posterior(bd, 20, seed=9, first_id=3)
        assert mean.is_cuda and samples.is_cuda
        mu = pkg.ldiv(F, bd)
        assert torch.equal(mean, mu)
        assert torch.equal(samples, F.sample(20, mean=mu, seed=9, first_id=3, like=bd))
        _check_mean_logdet(pkg, F, Q, rhs, nb, tol)
        _no_aborts(F)
    F.set_order("reference")                         # and back: the handle's own factor again, as a fresh handle has it
    F.factor(w.Q, N)
    assert F.stats()["persist_cus"] > 0
    mean, samples = F.posterior(b, 16, seed=2)
    F.close()
    R = pkg.tridiagonal_cholesky(w.Q, N)
    mean_r, samples_r = R.posterior(b, 16, seed=2)
    assert torch.equal(mean, mean_r) and torch.equal(samples, samples_r)
    R.close()


def test_refactor_values_host_and_device(pkg):
    """gmrf_bt_refactor_values on a twisted handle: host values (staged once for both halves) and device values (gathered by
    both halves and the meeting coupling from the caller's array) give the same bits, and the factor of the new values."""
    import torch
    w = pkg.workloads.make("darcy64")
    N = w.n_blocks
    tol = solve_tol(w)
    F = _twisted(pkg, w)
    mu0 = _check_mean_logdet(pkg, F, w.Q, w.rhs, N, tol)
    ld0 = F.logdet()
    Q2 = _shifted(w.Q, 0.25)
    F.refactor(Q2.data)
    mu_h = _check_mean_logdet(pkg, F, Q2, w.rhs, N, tol)          # (a raised diagonal: cond(Q2) <= cond(Q))
    ld_h, v_h = F.logdet(), F.marginal_var("exact")
    F.refactor(torch.from_numpy(Q2.data.copy()).cuda())
    assert np.array_equal(pkg.ldiv(F, w.rhs), mu_h) and F.logdet() == ld_h
    assert np.array_equal(F.marginal_var("exact"), v_h)
    assert rel(mu_h, mu0) > 1e-6                     # (the values did change)
    Q1 = sp.csc_matrix(w.Q, copy=True)
    Q1.sort_indices()
    F.refactor(Q1.data)
    assert np.array_equal(pkg.ldiv(F, w.rhs), mu0) and F.logdet() == ld0
    _no_aborts(F)
    F.close()
