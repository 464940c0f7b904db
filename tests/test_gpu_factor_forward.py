"""The forward solve inside a batch's factorisation (gmrf_bt_set_factor_rhs): with a registered right-hand side b the factor's own
products -- G2, the panel products, the rank-256 updates (gemm_f64_dma tail rows on [n][k] B, triangular grids with staircase
bounds, TRI_B_UPPER) -- also leave y = L^-1 b, and the fused posterior skips its forward sweep.  Checked: the factor is bitwise
unchanged, y against the forward sweep, the posterior against the two-call route and the oracle, the fallbacks, and the
abort-and-repeat of a persistent panel launch."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import __graft_entry__
from oracle import bt_oracle as O
from tests.test_gpu_parity import rel, solve_tol

pytestmark = pytest.mark.gpu

Switch = __graft_entry__.load_package().Switch
FORWARD = 1                  # gmrf_bt_solve mode: y = L^-1 b


def _leading(w, nb):
    m = nb * w.block_size
    Q = sp.csc_matrix(w.Q[:m, :m])
    Q.sort_indices()
    return Q, np.ascontiguousarray(w.rhs[:m]), nb


def _fwd_state(pkg, F, want_y=False):
    lib = pkg._cabi.load()
    st = C.c_int32(-1)
    y = np.empty((F.batch, F.N), dtype=np.float64) if want_y else None
    pkg._cabi.check(lib.gmrf_test_factor_fwd(F._h, C.byref(st), pkg._cabi.ptr(y) if want_y else None))
    return (int(st.value), y) if want_y else int(st.value)


def _fused(F):
    return F.stats()["sample_ms"] == 0.0


def _blocks(F, nb, probs):
    out = []
    for p in probs:
        F.select_problem(p)
        for i in range(nb):
            out.append(F.get_block(2, i))                  # Linv_i
            if i + 1 < nb:
                out.append(F.get_block(1, i))              # C_{i+1}
        out.append(np.array([F.logdet()]))
    F.select_problem(0)
    return out


# darcy256's leading blocks as a batch of 12 (persistent 256-column panels) and as a batch of 40 (potrf_diag128 + GEMMs);
# burgers512x64 as a batch of 16
CASES = {"darcy256_leading8_b12": ("darcy256", 8, 12), "darcy256_leading6_b40": ("darcy256", 6, 40),
         "burgers512x64_b16": ("burgers512x64", None, 16)}


@pytest.fixture(scope="module", params=list(CASES))
def fcase(request, pkg):
    import torch
    name, nb, B = CASES[request.param]
    w = pkg.workloads.make(name)
    if name == "darcy256":
        w.meta.setdefault("cond", 3.4e9)
    Q, rhs, nb = _leading(w, nb) if nb else (w.Q, w.rhs, w.n_blocks)
    vals = np.stack([Q.data * (1.0 + 0.05 * p) for p in range(B)])
    b = torch.from_numpy(np.stack([rhs * (1.0 + 0.5 * p) for p in range(B)])).cuda()
    F = pkg.TridiagonalCholeskyFactor(batch=B)
    F.set_factor_rhs(b)
    F.factor(Q, nb, values=vals)
    return w, Q, rhs, nb, B, F, vals, b


def test_factor_bitwise_unchanged_and_y_is_the_forward_sweep(pkg, fcase):
    w, Q, rhs, nb, B, F, vals, b = fcase
    st, y = _fwd_state(pkg, F, want_y=True)
    assert st == 1
    probs = (0, B - 1)
    with_rhs = _blocks(F, nb, probs)
    ysweep = F.solve_batch(b[:, None, :], mode=FORWARD)[:, 0, :].cpu().numpy()
    for p in range(B):
        assert rel(y[p], ysweep[p]) <= 1e-13
    # the same values without the forward solve: the same bits
    F.set_eager(Switch.NO_FACTOR_FWD)
    try:
        F.refactor(vals)
        assert _fwd_state(pkg, F) == 0
        without = _blocks(F, nb, probs)
    finally:
        F.set_eager(0)
        F.refactor(vals)
    assert _fwd_state(pkg, F) == 1
    assert len(with_rhs) == len(without)
    assert all(np.array_equal(a, c) for a, c in zip(with_rhs, without))


def test_posterior_with_the_factor_forward_solve(pkg, fcase):
    w, Q, rhs, nb, B, F, vals, b = fcase
    assert _fwd_state(pkg, F) == 1
    k, seed, first = 64, 91, 300
    mu_f, X_f = F.posterior_batch(b, k, seed=seed, first_id=first)
    assert _fused(F)
    # the L^-T z rows are gmrf_bt_sample's bits
    X_s = F.sample_batch(k, mean=mu_f, seed=seed, first_id=first, like=b)
    assert bool((X_s == X_f).all())
    # the two-call route (eager bit 18) to rounding
    F.set_eager(Switch.TWO_CALL_POSTERIOR)
    try:
        mu_u, X_u = F.posterior_batch(b, k, seed=seed, first_id=first)
    finally:
        F.set_eager(0)
        F.refactor(vals)
    mu_f_h, mu_u_h = mu_f.cpu().numpy(), mu_u.cpu().numpy()
    for p in range(B):
        assert rel(mu_f_h[p], mu_u_h[p]) < 1e-12
    # the oracle
    tol = solve_tol(w)
    for p in (0, B - 1):
        Qp = Q.copy(); Qp.data = vals[p]
        Fo = O.tridiagonal_cholesky(Qp, nb)
        mu_o = O.ldiv(Fo, rhs * (1.0 + 0.5 * p))
        assert rel(mu_f_h[p], mu_o) < tol


def test_fallbacks_run_the_forward_sweep(pkg, fcase):
    import torch
    w, Q, rhs, nb, B, F, vals, b = fcase
    k, seed, first = 64, 5, 0
    assert _fwd_state(pkg, F) == 1
    mu_ref, X_ref = F.posterior_batch(b, k, seed=seed, first_id=first)
    mu_ref, X_ref = mu_ref.cpu().numpy(), X_ref.cpu().numpy()
    # another pointer with the same values: the forward sweep runs, the same results to rounding (the mean of the other
    # handles below too: cond(Q) times eps, as against the two-call route)
    b2 = b.clone()
    mu2, X2 = F.posterior_batch(b2, k, seed=seed, first_id=first)
    assert _fused(F)
    for p in range(B):
        assert rel(mu2[p].cpu().numpy(), mu_ref[p]) < 1e-10
    # a factor without a registered right-hand side
    G = pkg.TridiagonalCholeskyFactor(batch=B)
    G.factor(Q, nb, values=vals)
    assert _fwd_state(pkg, G) == 0
    mu3, _ = G.posterior_batch(b, k, seed=seed, first_id=first)
    for p in range(B):
        assert rel(mu3[p].cpu().numpy(), mu_ref[p]) < 1e-10
    # registered, then cleared: the next factor leaves no y
    G.set_factor_rhs(b)
    G.refactor(vals)
    assert _fwd_state(pkg, G) == 1
    G.set_factor_rhs(None)
    G.refactor(vals)
    assert _fwd_state(pkg, G) == 0
    # stepwise factorisation (the shared-factor path): no y
    G.set_factor_rhs(b)
    G.factor_begin_values(torch.from_numpy(vals).cuda())
    G.factor_step_async(0, nb)
    G.factor_end()
    assert _fwd_state(pkg, G) == 0
    mu4, _ = G.posterior_batch(b, k, seed=seed, first_id=first)
    for p in range(B):
        assert rel(mu4[p].cpu().numpy(), mu_ref[p]) < 1e-10


def test_one_problem_and_twisted_leave_no_y(pkg):
    import torch
    w = pkg.workloads.make("darcy64")
    b = torch.from_numpy(np.ascontiguousarray(w.rhs)[None, :]).cuda()
    F = pkg.TridiagonalCholeskyFactor()
    F.set_factor_rhs(b)
    F.factor(w.Q, w.n_blocks)
    assert _fwd_state(pkg, F) == 0
    mu = pkg.ldiv(F, w.rhs)
    T = pkg.TridiagonalCholeskyFactor()
    T.set_order("twisted")
    T.set_factor_rhs(b)
    T.factor(w.Q, w.n_blocks)
    assert _fwd_state(pkg, T) == 0
    assert rel(pkg.ldiv(T, w.rhs), mu) < 1e-10


def test_persistent_panel_abort_recomputes_y(pkg):
    """A persistent panel launch that gives up (GMRF_PERSIST_SPIN_MS=0, in a child process) is repeated launch-per-step; the
    repeat re-runs the blocks' launches, the forward solve's included: the posterior's mean is still right."""
    env = dict(os.environ, GMRF_PERSIST_SPIN_MS="0")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "factor_forward_abort_child.py")], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["aborts"] == 1 and out["fwd"] == 1, out
    assert out["mean_rel"] < 1e-12 and out["y_rel"] <= 1e-13, out
