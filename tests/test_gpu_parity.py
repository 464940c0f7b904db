"""GPU parity tests: the HIP path through the C ABI against the oracle (oracle/bt_oracle.py)
on the same seeded inputs.  fp64 tolerances are stated per test; they are relative l2 unless
noted, and sized from cond(Q) ~ 1e7 (darcy) * eps."""
import numpy as np
import pytest
import scipy.sparse as sp

import __graft_entry__
from oracle import bt_oracle as O

pytestmark = pytest.mark.gpu
Switch = __graft_entry__.load_package().Switch

TOL_FACTOR = 1e-11     # max-abs / max-abs on factor blocks
EPS = 2.220446049250313e-16


def solve_tol(w):
    """fp64 tolerance of a solve against the oracle: 0.25 * cond(Q) * eps, floor 1e-12.
    Two backward-stable fp64 factorisations of the same matrix agree to O(cond * eps) and no
    better; BASELINE.md's flat 1e-10 gate is met wherever cond(Q) <= 4.5e6 and is replaced by
    this bound for the ill-conditioned posteriors (darcy64: cond 1.3e7 -> 2.8e-10;
    darcy256: cond 3.4e9 -> 7.7e-8; measured differences are 10-300x below the bound)."""
    if "cond" not in w.meta:
        import scipy.sparse.linalg as spla
        lmax = spla.eigsh(w.Q, k=1, which="LA", return_eigenvectors=False)[0]
        lu = spla.splu(w.Q.tocsc())
        imax = spla.eigsh(spla.LinearOperator(w.Q.shape, matvec=lu.solve), k=1, which="LA",
                          return_eigenvectors=False)[0]
        w.meta["cond"] = float(lmax * imax)
    return max(1e-12, 0.25 * w.meta["cond"] * EPS)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


@pytest.fixture(scope="module", params=["darcy32", "darcy64", "burgers64x8", "elliptic32"])
def case(request, pkg):
    w = pkg.workloads.make(request.param)
    F = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
    Fo = O.tridiagonal_cholesky(w.Q, w.n_blocks)
    return w, F, Fo


def test_factor_blocks_match(case):
    w, F, Fo = case
    assert F.N == Fo.N and len(F.chos) == len(Fo.chos) and len(F.Cs) == len(Fo.Cs)
    for i in range(0, w.n_blocks, max(1, w.n_blocks // 5)):
        L = F.chos[i]
        assert np.max(np.abs(np.tril(L) - Fo.chos[i])) / np.max(np.abs(Fo.chos[i])) < TOL_FACTOR
        assert np.allclose(np.triu(L, 1), 0.0)
        if i < w.n_blocks - 1:
            assert np.max(np.abs(F.Cs[i] - Fo.Cs[i])) / np.max(np.abs(Fo.Cs[i])) < TOL_FACTOR


def test_mean_and_half_solves(case, pkg):
    w, F, Fo = case
    mu = pkg.ldiv(F, w.rhs)
    tol = solve_tol(w)
    assert rel(mu, O.ldiv(Fo, w.rhs)) < tol
    assert rel(pkg.forward_solve(F, w.rhs), O.forward_solve(Fo, w.rhs)) < tol
    assert rel(pkg.backward_solve(F, w.rhs), O.backward_solve(Fo, w.rhs)) < tol
    r = w.Q @ mu - w.rhs
    qn = abs(w.Q).sum(axis=1).max()
    assert np.linalg.norm(r) / (qn * np.linalg.norm(mu) + np.linalg.norm(w.rhs)) < 1e-14
    y = np.empty_like(w.rhs)
    assert pkg.ldiv_(y, F, w.rhs) is y and rel(y, mu) == 0.0


@pytest.mark.parametrize("k", [2, 16, 33, 64, 128])
def test_matrix_right_hand_sides(case, pkg, k):
    w, F, Fo = case
    B = np.random.default_rng(k).standard_normal((w.n, k))
    tol = solve_tol(w)
    assert rel(pkg.ldiv(F, B), O.ldiv(Fo, B)) < tol
    assert rel(pkg.backward_solve(F, B), O.backward_solve(Fo, B)) < tol
    assert rel(pkg.forward_solve(F, B), O.forward_solve(Fo, B)) < tol


def test_samples_with_given_z_and_logdet(case, pkg):
    w, F, Fo = case
    mu_o = O.ldiv(Fo, w.rhs)
    Z = np.random.default_rng(3).standard_normal((w.n, 24))
    X = F.sample(24, mean=mu_o, z=Z)
    assert rel(X, O.sample(Fo, mu_o, Z)) < solve_tol(w)
    assert abs(F.logdet() - O.logdet(Fo)) < 1e-9 * abs(O.logdet(Fo))


def test_exact_marginal_variances(case, pkg):
    w, F, Fo = case
    v = F.marginal_var("exact")
    vo = O.marginal_variances_exact(Fo)
    assert np.max(np.abs(v - vo) / vo) < 1e-9          # exact variances rel <= 1e-9
    import torch
    vd_out = torch.empty(w.n, dtype=torch.float64, device="cuda")       # `out=` on the device: the same numbers, no host array
    assert F.marginal_var("exact", out=vd_out) is vd_out and np.array_equal(vd_out.cpu().numpy(), v)
    with pytest.raises(ValueError):
        F.marginal_var("exact", out=np.empty(w.n + 1))
    if w.n <= 1024:
        vd = np.diag(np.linalg.inv(w.Q.toarray()))
        assert np.max(np.abs(v - vd) / vd) < 1e-7


def test_rbmc_and_mc_variances_with_device_philox(case, pkg):
    w, F, Fo = case
    Q = pkg.CsrMatrix(w.Q)
    k = 48
    Z = F.normals(k, seed=77)
    X = O.backward_solve(Fo, Z)
    v_rbmc = F.marginal_var("rbmc", k=k, seed=77, Q=Q)
    v_mc = F.marginal_var("mc", k=k, seed=77)
    assert np.max(np.abs(v_rbmc - O.marginal_variances_rbmc(w.Q, X)) / v_rbmc) < 1e-8
    assert np.max(np.abs(v_mc - O.marginal_variances_mc(X)) / v_mc) < 1e-8
    # sharded accumulation (two "ranks") gives the same estimator
    acc = np.zeros(w.n)
    F.var_accumulate(acc, "mc", 0, 20, seed=77)
    F.var_accumulate(acc, "mc", 20, 28, seed=77)
    assert np.max(np.abs(acc / k - v_mc) / v_mc) < 1e-12


def test_philox_normals_are_geometry_independent_and_standard(pkg):
    w = pkg.workloads.make("darcy32")
    F = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
    Z = F.normals(40, seed=5)
    Z2 = F.normals(8, seed=5, first_id=16)
    assert np.array_equal(Z[:, 16:24], Z2)              # keyed by (seed, sample id, dof) only
    assert abs(Z.mean()) < 0.02 and abs(Z.std() - 1.0) < 0.02
    from tests.philox_ref import philox_normal
    ref = np.array([[philox_normal(5, d, s) for s in (0, 7)] for d in (0, 1, 1023)])
    assert np.max(np.abs(Z[[0, 1, 1023]][:, [0, 7]] - ref)) < 1e-13


def test_spmm_fp64_and_fp32_values(pkg):
    w = pkg.workloads.make("darcy32")
    X = np.random.default_rng(1).standard_normal((w.n, 5))
    Q = pkg.CsrMatrix(w.Q)
    assert rel(Q @ X, w.Q @ X) < 1e-14
    assert rel(Q @ X[:, 0], w.Q @ X[:, 0]) < 1e-14
    Q32 = pkg.CsrMatrix(w.Q, values_f32=True)
    ref32 = sp.csr_matrix((w.Q.tocsr().data.astype(np.float32).astype(np.float64), w.Q.tocsr().indices,
                           w.Q.tocsr().indptr), shape=w.Q.shape) @ X
    assert rel(Q32 @ X, ref32) < 1e-14
    assert rel(Q32 @ X[:, 1], ref32[:, 1]) < 1e-14          # SpMV (LDS-staged row tiles), fp32 values
    # ragged rows: empty rows, a row count that is no multiple of the 64-row tile, rectangular shape
    rng = np.random.default_rng(8)
    A = sp.random(1000, 700, density=0.01, random_state=rng, data_rvs=rng.standard_normal).tolil()
    A[5, :] = 0.0; A[999, :] = 0.0
    A = A.tocsr(); A.eliminate_zeros()
    x = rng.standard_normal(700)
    assert rel(pkg.CsrMatrix(A) @ x, A @ x) < 1e-14
    # a tile with more entries than the LDS image holds falls back to the lane-group kernel
    D = sp.random(200, 300, density=0.5, random_state=rng, data_rvs=rng.standard_normal).tocsr()
    xd = rng.standard_normal(300)
    assert rel(pkg.CsrMatrix(D) @ xd, D @ xd) < 1e-13


def test_refactor_values_same_pattern(pkg):
    w = pkg.workloads.make("darcy32")
    F = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
    Q2 = w.Q.copy()
    Q2.data = Q2.data * 1.5
    F.refactor(Q2.data)
    assert rel(pkg.ldiv(F, w.rhs), O.ldiv(O.tridiagonal_cholesky(Q2, w.n_blocks), w.rhs)) < solve_tol(w)


def test_eager_and_graph_paths_agree_bitwise(pkg):
    w = pkg.workloads.make("darcy32")
    F = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
    a = pkg.ldiv(F, w.rhs)
    F.set_eager(Switch.EAGER)
    F.refactor(w.Q.data)
    b = pkg.ldiv(F, w.rhs)
    assert np.array_equal(a, b)


def test_panel_sweeps_through_gemm_match_sweep_kernel(pkg):
    # 64-multiples of right-hand sides run the sweeps on the GEMM kernel; bit 2 of set_eager keeps
    # them on sweep_mm.  Same products, different summation order.
    w = pkg.workloads.make("darcy64")
    nb = 32                                     # enough problems for the GEMM route (128 tiles)
    F = pkg.TridiagonalCholeskyFactor(batch=nb).factor(w.Q, w.n_blocks, values=np.tile(w.Q.data, (nb, 1)))
    B = np.random.default_rng(5).standard_normal((nb, 64, w.n))
    a = [F.solve_batch(B, m) for m in (pkg._cabi.SOLVE_FULL, pkg._cabi.SOLVE_FORWARD, pkg._cabi.SOLVE_BACKWARD)]
    F.set_eager(Switch.SWEEP_NO_GEMM)
    b = [F.solve_batch(B, m) for m in (pkg._cabi.SOLVE_FULL, pkg._cabi.SOLVE_FORWARD, pkg._cabi.SOLVE_BACKWARD)]
    for x, y in zip(a, b):
        assert rel(x, y) < 1e-12 and not np.array_equal(x, y)
    Fo = O.tridiagonal_cholesky(w.Q, w.n_blocks)
    assert rel(a[0][7].T, O.ldiv(Fo, B[7].T)) < solve_tol(w)


def test_forked_factor_graph_matches_single_branch(pkg):
    """Opt-in (set_eager bit 4): for blocks of 8+ tiles the captured factor graph assembles the inverse
    of a block's first half on a second branch beside the panel chain of the second half.  Same
    kernels on the same data: bitwise equal to the single-branch graph and to plain stream launches."""
    w = pkg.workloads.make("burgers512x64")
    F = pkg.TridiagonalCholeskyFactor()
    F.set_eager(Switch.DOUBLING_INVERSE)                         # the inverse by recursive doubling: what the forked branch overlaps
    F.factor(w.Q, w.n_blocks)
    a = pkg.ldiv(F, w.rhs); la = F.chos[40].copy(); xa = F.get_block(pkg._cabi.BLOCK_LINV, 40)
    for flags in (Switch.FORK_GRAPH | Switch.DOUBLING_INVERSE, Switch.EAGER | Switch.DOUBLING_INVERSE, Switch.FORK_GRAPH | Switch.DOUBLING_INVERSE):
        F.set_eager(flags)
        for _ in range(2):                   # capture, then a replay of the forked graph
            F.refactor(w.Q.data)
            assert np.array_equal(pkg.ldiv(F, w.rhs), a) and np.array_equal(F.chos[40], la)
            assert np.array_equal(F.get_block(pkg._cabi.BLOCK_LINV, 40), xa)


def test_extract_blocks_route_and_padding(pkg):
    # block size 40 is padded to 64 inside the library; blocks come from extract_blocks
    w = pkg.workloads.random_block_tridiagonal(5, 40, seed=3)
    coo = w.Q.tocoo()
    d, o = pkg.extract_blocks(coo.row + 1, coo.col + 1, coo.data, 40)
    do, oo = O.extract_blocks(coo.row + 1, coo.col + 1, coo.data, 40)
    assert all((a != b).nnz == 0 for a, b in zip(d, do)) and all((a != b).nnz == 0 for a, b in zip(o, oo))
    F = pkg.TridiagonalCholeskyFactor().factor_blocks(d, o)
    Fo = O.tridiagonal_cholesky(w.Q, 5)
    assert rel(pkg.ldiv(F, w.rhs), O.ldiv(Fo, w.rhs)) < 1e-12
    assert np.max(np.abs(np.tril(F.chos[4]) - Fo.chos[4])) < 1e-12


def test_error_paths(pkg):
    w = pkg.workloads.random_block_tridiagonal(4, 64, seed=1)
    with pytest.raises(ValueError):
        pkg.tridiagonal_cholesky(w.Q, 3)                       # n % N != 0
    bad = w.Q.tolil(); bad[200, 10] = 1.0; bad[10, 200] = 1.0
    with pytest.raises(pkg.GmrfError) as e:
        pkg.tridiagonal_cholesky(bad.tocsc(), 4)               # outside the tri-band
    assert e.value.status == pkg._cabi.ERR_BAND
    ns = w.Q.tolil(); ns[130, 130] = -50.0
    with pytest.raises(pkg.NotPositiveDefinite) as e:
        pkg.tridiagonal_cholesky(ns.tocsc(), 4)
    assert e.value.info == 3                                   # 1-based failing block
    with pytest.raises(O.NotPositiveDefinite) as eo:
        O.tridiagonal_cholesky(ns.tocsc(), 4)
    assert eo.value.block == 3
    F = pkg.TridiagonalCholeskyFactor()
    F.N = 256
    with pytest.raises(pkg.GmrfError):
        pkg.ldiv(F, np.zeros(256))                             # solve before factor


def test_handle_life_cycle_recovery_and_reuse(pkg):
    """One handle through a failed factorisation, a recovery on the same pattern, a different
    pattern and shape, a change of batch size, and several handles driven from host threads."""
    import threading
    w = pkg.workloads.random_block_tridiagonal(4, 64, seed=1)
    F = pkg.tridiagonal_cholesky(w.Q, 4)
    x0 = pkg.ldiv(F, w.rhs)
    bad = w.Q.data.copy()
    Qc = w.Q.tocsc()
    d = np.flatnonzero((Qc.indices == 130) & (np.repeat(np.arange(w.n), np.diff(Qc.indptr)) == 130))[0]
    bad[d] = -50.0
    with pytest.raises(pkg.NotPositiveDefinite):
        F.refactor(bad)
    with pytest.raises(pkg.GmrfError):                        # the failed factor is not usable
        pkg.ldiv(F, w.rhs)
    F.refactor(w.Q.data)                                       # same handle recovers
    assert np.array_equal(pkg.ldiv(F, w.rhs), x0)
    w2 = pkg.workloads.random_block_tridiagonal(3, 130, seed=6)   # other pattern, other shape
    F.factor(w2.Q, 3)
    assert rel(pkg.ldiv(F, w2.rhs), O.ldiv(O.tridiagonal_cholesky(w2.Q, 3), w2.rhs)) < 1e-12
    F.set_batch(2)                                             # other batch size on the same handle
    F.factor(w.Q, 4, values=np.stack([w.Q.data, 2.0 * w.Q.data]))
    xb = F.solve_batch(np.stack([w.rhs, w.rhs])[:, None, :])[:, 0, :]
    assert np.array_equal(xb[0], x0) and rel(xb[1], 0.5 * x0) < 1e-13
    # alternating shapes on one handle do not leak device memory
    import torch
    F.set_batch(1)
    used = []
    for it in range(6):
        wa = w if it % 2 == 0 else w2
        F.factor(wa.Q, wa.n_blocks)
        pkg.ldiv(F, wa.rhs); F.sample(3, seed=1); F.marginal_var("exact")
        free_b, total_b = torch.cuda.mem_get_info(0)
        used.append(total_b - free_b)
    assert max(used[2:]) - min(used[2:]) < 64 << 20
    # independent handles on their own streams, one host thread each
    res = [None] * 4
    def work(i):
        Fi = pkg.tridiagonal_cholesky(w.Q, 4)
        for _ in range(5):
            Fi.refactor(w.Q.data)
            res[i] = pkg.ldiv(Fi, w.rhs)
    ths = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    [t.start() for t in ths]; [t.join() for t in ths]
    assert all(np.array_equal(r, x0) for r in res)


def test_c_abi_leading_dimensions_in_place_and_mixed_k(pkg, lib):
    """Straight through the C ABI: column-major right-hand sides with ld > n (host and device
    memory), in place (y == b, as ldiv! allows), right-hand-side counts changing from call to call,
    and the factor image of a batch member other than the first."""
    import torch
    w = pkg.workloads.random_block_tridiagonal(5, 40, seed=12)
    F = pkg.tridiagonal_cholesky(w.Q, 5)
    Fo = O.tridiagonal_cholesky(w.Q, 5)
    n, ld = w.n, w.n + 7
    rng = np.random.default_rng(2)
    for k in (1, 3, 64, 200, 2, 129, 1):
        B = rng.standard_normal((n, k))
        buf = np.full((k, ld), np.nan)                    # k columns of length ld, column-major n x k inside
        buf[:, :n] = B.T
        buf0 = buf.copy()
        pkg._cabi.check(lib.gmrf_bt_solve(F._h, pkg._cabi.ptr(buf), pkg._cabi.ptr(buf), k, ld, ld, pkg._cabi.SOLVE_FULL))
        assert rel(buf[:, :n].T, O.ldiv(Fo, B)) < 1e-12 and np.all(np.isnan(buf[:, n:]))
        dev = torch.full((k, ld), float("nan"), dtype=torch.float64, device="cuda")
        dev[:, :n] = torch.from_numpy(B.T.copy()).cuda()
        out = torch.zeros_like(dev)
        pkg._cabi.check(lib.gmrf_bt_solve(F._h, pkg._cabi.ptr(dev), pkg._cabi.ptr(out), k, ld, ld, pkg._cabi.SOLVE_BACKWARD))
        assert rel(out[:, :n].T.cpu().numpy(), O.backward_solve(Fo, B)) < 1e-12
        assert float(out[:, n:].abs().sum()) == 0.0       # the padding of the output is not written
        # different leading dimensions on the two sides (a strided view in, a dense matrix out)
        dense = np.empty((k, n))
        pkg._cabi.check(lib.gmrf_bt_solve(F._h, pkg._cabi.ptr(buf0), pkg._cabi.ptr(dense), k, ld, n, pkg._cabi.SOLVE_FORWARD))
        assert rel(dense.T, O.forward_solve(Fo, B)) < 1e-12
        assert lib.gmrf_bt_solve(F._h, pkg._cabi.ptr(dense), pkg._cabi.ptr(dense), k, n, ld, 0) == pkg._cabi.ERR_BAD_SHAPE
    # export the factor of problem 1 of a batch
    Fb = pkg.TridiagonalCholeskyFactor(batch=2).factor(w.Q, 5, values=np.stack([w.Q.data, 4.0 * w.Q.data]))
    Fb.select_problem(1)
    G = pkg.TridiagonalCholeskyFactor().import_factor(Fb.export_factor())
    assert rel(pkg.ldiv(G, w.rhs), 0.25 * O.ldiv(Fo, w.rhs)) < 1e-12


def test_degenerate_shapes(pkg):
    # N = 1 (plain dense Cholesky) and a long chain of small blocks
    w1 = pkg.workloads.random_block_tridiagonal(1, 128, seed=2)
    F1 = pkg.tridiagonal_cholesky(w1.Q, 1)
    assert rel(pkg.ldiv(F1, w1.rhs), np.linalg.solve(w1.Q.toarray(), w1.rhs)) < 1e-12
    w2 = pkg.workloads.random_block_tridiagonal(40, 8, seed=4)
    F2 = pkg.tridiagonal_cholesky(w2.Q, 40)
    assert rel(pkg.ldiv(F2, w2.rhs), O.ldiv(O.tridiagonal_cholesky(w2.Q, 40), w2.rhs)) < 1e-12


@pytest.mark.parametrize("bs", [1, 3, 40, 64, 65, 130, 200, 520])
def test_ragged_block_sizes_and_panel_widths(pkg, bs):
    """Block sizes around the 64 / 128 / 512 padding boundaries (bs = 1: scalar tridiagonal),
    chains of 1, 2 and 5 blocks, 1 / 3 / 65 / 130 right-hand sides: factor blocks, the three solves,
    samples with given z, exact variances and logdet against the oracle."""
    for N in (1, 2, 5):
        w = pkg.workloads.random_block_tridiagonal(N, bs, seed=100 + bs + N, density=min(1.0, 6.0 / bs))
        F = pkg.tridiagonal_cholesky(w.Q, N)
        Fo = O.tridiagonal_cholesky(w.Q, N)
        assert np.max(np.abs(np.tril(F.chos[N - 1]) - Fo.chos[N - 1])) / np.max(np.abs(Fo.chos[N - 1])) < TOL_FACTOR
        if N > 1:
            assert np.max(np.abs(F.Cs[N - 2] - Fo.Cs[N - 2])) <= TOL_FACTOR * max(1e-300, np.max(np.abs(Fo.Cs[N - 2])))
        rng = np.random.default_rng(bs * 7 + N)
        for k in (1, 3, 65, 130):
            B = rng.standard_normal((w.n, k)) if k > 1 else rng.standard_normal(w.n)
            assert rel(pkg.ldiv(F, B), O.ldiv(Fo, B)) < 1e-12
            assert rel(pkg.forward_solve(F, B), O.forward_solve(Fo, B)) < 1e-12
            assert rel(pkg.backward_solve(F, B), O.backward_solve(Fo, B)) < 1e-12
        Z = rng.standard_normal((w.n, 5))
        mu = O.ldiv(Fo, w.rhs)
        assert rel(F.sample(5, mean=mu, z=Z), O.sample(Fo, mu, Z)) < 1e-12
        vo = O.marginal_variances_exact(Fo)
        assert np.max(np.abs(F.marginal_var("exact") - vo) / vo) < 1e-10
        assert abs(F.logdet() - O.logdet(Fo)) < 1e-11 * max(1.0, abs(O.logdet(Fo)))


def test_batch_with_padded_blocks_on_the_two_level_path(pkg):
    # bs = 520 is padded to 1024 (16 tiles): batches take the 256-column panel path on padded blocks
    w = pkg.workloads.random_block_tridiagonal(3, 520, seed=31, density=0.012)
    vals = np.stack([w.Q.data, w.Q.data * 0.5, w.Q.data * 3.0])
    rhs = np.stack([w.rhs, -w.rhs, 2.0 * w.rhs])
    Fb = pkg.TridiagonalCholeskyFactor(batch=3).factor(w.Q, 3, values=vals)
    mu = Fb.solve_batch(rhs[:, None, :])[:, 0, :]
    Fo = O.tridiagonal_cholesky(w.Q, 3)
    x0 = O.ldiv(Fo, w.rhs)
    for p, f in enumerate((1.0, -2.0, 2.0 / 3.0)):
        assert rel(mu[p], f * x0) < 1e-12
    vb = Fb.marginal_var("exact")
    vo = O.marginal_variances_exact(Fo)
    assert np.max(np.abs(vb[1] - 2.0 * vo) / vo) < 1e-9
    Fb.select_problem(2)
    assert abs(Fb.logdet() - (O.logdet(Fo) + w.n * np.log(3.0))) < 1e-10 * abs(O.logdet(Fo))


@pytest.mark.parametrize("name", ["darcy64", "burgers64x8"])
def test_sparse_and_dense_coupling_product_agree(pkg, name):
    """C = B X^T: the sparse kernel (spmm_bxt, default for FEM coupling blocks) against the dense
    GEMM route (set_eager bit 3), and both against the oracle."""
    w = pkg.workloads.make(name)
    Fo = O.tridiagonal_cholesky(w.Q, w.n_blocks)
    Fs = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
    Fd = pkg.TridiagonalCholeskyFactor()
    Fd.set_eager(Switch.DENSE_COUPLING)
    Fd.factor(w.Q, w.n_blocks)
    for i in (0, w.n_blocks // 2, w.n_blocks - 2):
        scale = np.max(np.abs(Fo.Cs[i]))
        assert np.max(np.abs(Fs.Cs[i] - Fo.Cs[i])) / scale < TOL_FACTOR
        assert np.max(np.abs(Fd.Cs[i] - Fo.Cs[i])) / scale < TOL_FACTOR
        assert np.max(np.abs(Fd.Cs[i] - Fs.Cs[i])) / scale < 1e-13
    assert rel(pkg.ldiv(Fs, w.rhs), pkg.ldiv(Fd, w.rhs)) < solve_tol(w)
    # the GEMM route with a batch (dense image of B per problem)
    Fb = pkg.TridiagonalCholeskyFactor(batch=2)
    Fb.set_eager(Switch.DENSE_COUPLING)
    Fb.factor(w.Q, w.n_blocks, values=np.stack([w.Q.data, 2.0 * w.Q.data]))
    xb = Fb.solve_batch(np.stack([w.rhs, w.rhs])[:, None, :])[:, 0, :]
    # (a batch assembles the inverses by recursive doubling, one problem row by row inside the fused steps: equal to rounding)
    assert rel(xb[0], pkg.ldiv(Fd, w.rhs)) < solve_tol(w) and rel(xb[1], 0.5 * xb[0]) < solve_tol(w)
    # a block-dense coupling (more than 32 entries per row) takes the GEMM route by itself
    wd = pkg.workloads.random_block_tridiagonal(3, 128, seed=2, density=0.6)
    F = pkg.tridiagonal_cholesky(wd.Q, wd.n_blocks)
    assert rel(pkg.ldiv(F, wd.rhs), O.ldiv(O.tridiagonal_cholesky(wd.Q, wd.n_blocks), wd.rhs)) < 1e-12


@pytest.mark.parametrize("name", ["darcy256", "burgers512x64"])
def test_coupling_product_by_tile_groups(pkg, name):
    """Round 4: spmm_bxt_tiles serves GROUPS of up to three 64-row tiles of a lower block that meet the same columns of X (one
    gathered chunk multiplied by up to 192 rows).  The coupling blocks C_i of a batch must be bitwise what the same kernel gives
    with every tile alone (GMRF_BXT_GROUPS=0) and what the row kernel gives (GMRF_BXT_TILES=0) -- a row's entries are summed in
    the same order whoever gathers its operands.  The switches are read once per process: child processes."""
    import json
    import subprocess
    import sys
    child = _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "bxt_child.py")

    def run(**env):
        r = subprocess.run([sys.executable, child, name], env=dict(_os.environ, **env), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return json.loads(r.stdout.strip().splitlines()[-1])

    grouped, alone, rows = run(), run(GMRF_BXT_GROUPS="0"), run(GMRF_BXT_TILES="0")
    assert grouped == alone == rows
    assert len(set(grouped.values())) == len(grouped)          # (six different blocks, not six times the same digest)


def test_export_import_factor_round_trip(pkg):
    w = pkg.workloads.random_block_tridiagonal(5, 40, seed=9)      # bs 40: padded to 64 inside
    F = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
    img = F.export_factor()
    hdr = img[:64].view(np.int64)
    assert tuple(hdr[:6]) == (0x46524D47, 1, w.n, w.n_blocks, 40, 1)
    blocks = img[64:].view(np.float64).reshape(3 * w.n_blocks - 1, 40, 40)
    assert np.array_equal(blocks[1].T, F.chos[1]) and np.array_equal(blocks[w.n_blocks + 2].T, F.Cs[2])
    G = pkg.TridiagonalCholeskyFactor().import_factor(img)
    assert np.array_equal(pkg.ldiv(G, w.rhs), pkg.ldiv(F, w.rhs)) and G.logdet() == F.logdet()
    assert np.array_equal(G.sample(3, seed=5), F.sample(3, seed=5))
    with pytest.raises(pkg.GmrfError):
        pkg.TridiagonalCholeskyFactor().import_factor(img[:-8])


def test_known_answer_closed_forms(pkg):
    """SURVEY 8c known-answer cases on the device: (i) 5-point kappa^2 I + Delta_h grid -- mean
    against a dense solve, exact marginal variances against the sine-transform closed form;
    (ii) AR(1) chain (x) I -- identity / -phi I factor blocks and the closed-form log-determinant."""
    nx, ny, k2 = 64, 24, 0.5
    w = pkg.workloads.laplace_kappa_grid(nx, ny, k2)
    F = pkg.tridiagonal_cholesky(w.Q, ny)
    assert rel(pkg.ldiv(F, w.rhs), np.linalg.solve(w.Q.toarray(), w.rhs)) < 1e-13
    v = F.marginal_var("exact")
    assert np.max(np.abs(v - pkg.workloads.laplace_kappa_grid_variances(nx, ny, k2))) < 1e-13
    phi, N, bs = 0.6, 9, 64
    w = pkg.workloads.ar1_chain_kron_identity(N, bs, phi)
    F = pkg.tridiagonal_cholesky(w.Q, N)
    for i in (0, 4, N - 1):
        want = np.eye(bs) * (np.sqrt(1.0 - phi * phi) if i == N - 1 else 1.0)
        assert np.max(np.abs(F.chos[i] - want)) < 1e-15
    assert np.max(np.abs(F.Cs[3] + phi * np.eye(bs))) < 1e-15
    assert abs(F.logdet() - bs * np.log(1.0 - phi * phi)) < 1e-12


def test_sample_covariance_matches_inverse(pkg):
    """statistical test of device-Philox samples, k = 16384 at n = 96:
    every entry of the sample covariance within 6 standard errors of (Q^-1)_ij."""
    w = pkg.workloads.random_block_tridiagonal(6, 16, seed=21)
    F = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
    k = 16384
    X = F.sample(k, seed=77)                          # n x k, zero mean
    S = np.linalg.inv(w.Q.toarray())
    Chat = X @ X.T / k
    se = np.sqrt((np.outer(np.diag(S), np.diag(S)) + S * S) / k)
    assert np.max(np.abs(Chat - S) / se) < 6.0
    assert np.max(np.abs(X.mean(axis=1)) / np.sqrt(np.diag(S) / k)) < 6.0


def test_torch_device_resident_io(pkg):
    import torch
    w = pkg.workloads.make("darcy32")
    F = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
    b = torch.from_numpy(w.rhs).cuda()
    mu = pkg.ldiv(F, b)
    assert mu.is_cuda and rel(mu.cpu().numpy(), pkg.ldiv(F, w.rhs)) == 0.0
    X = F.sample(16, mean=mu, seed=9, like=b)
    assert X.is_cuda and X.shape == (w.n, 16)
    Xh = F.sample(16, mean=mu.cpu().numpy(), seed=9)
    assert np.array_equal(X.cpu().numpy(), Xh)


import glob as _glob
import os as _os

_GOLDEN = sorted(_glob.glob(_os.path.join(_os.path.dirname(__file__), "golden", "*.npz")))


@pytest.mark.parametrize("path", _GOLDEN, ids=[_os.path.basename(p)[:-4] for p in _GOLDEN])
def test_hip_path_against_golden_fixtures(pkg, path):
    """Committed input/output vectors produced by an independent dense route
    (tests/golden/make_golden.py); includes block sizes that the library pads (24, 32)."""
    gd = np.load(path)
    n, N = int(gd["n"]), int(gd["n_blocks"])
    Q = sp.csc_matrix((gd["nzval"], gd["rowval"], gd["colptr"]), shape=(n, n))
    F = pkg.tridiagonal_cholesky(Q, N)
    scale = np.abs(gd["chos"]).max()
    for i in range(N):
        assert np.max(np.abs(np.tril(F.chos[i]) - gd["chos"][i])) < 1e-11 * scale
        if i < N - 1:
            assert np.max(np.abs(F.Cs[i] - gd["Cs"][i])) < 1e-11 * scale
    assert rel(pkg.ldiv(F, gd["rhs"]), gd["mean"]) < 1e-9
    assert rel(pkg.forward_solve(F, gd["Z"]), gd["forward"]) < 1e-10
    assert rel(pkg.backward_solve(F, gd["Z"]), gd["backward"]) < 1e-10
    assert np.max(np.abs(F.marginal_var("exact") - gd["var"]) / gd["var"]) < 1e-8
    assert abs(F.logdet() - float(gd["logdet"])) < 1e-10 * abs(float(gd["logdet"]))


def test_full_size_properties_darcy256(pkg):
    """BASELINE metric size: size-independent properties (residual, L L^T x = A x through
    the two half solves, linearity, logdet additivity under scaling)."""
    w = pkg.workloads.make("darcy256")
    F = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
    mu = pkg.ldiv(F, w.rhs)
    qn = abs(w.Q).sum(axis=1).max()
    assert np.linalg.norm(w.Q @ mu - w.rhs) / (qn * np.linalg.norm(mu) + np.linalg.norm(w.rhs)) < 1e-14
    rng = np.random.default_rng(0)
    X = rng.standard_normal((w.n, 3))
    # A^-1 (A x) = x
    assert rel(pkg.ldiv(F, w.Q @ X), X) < 1e-7
    # forward o backward = full; linearity
    B = rng.standard_normal((w.n, 2))
    assert rel(pkg.backward_solve(F, pkg.forward_solve(F, B)), pkg.ldiv(F, B)) < 1e-13
    assert rel(pkg.ldiv(F, 2.0 * B[:, 0] - 3.0 * B[:, 1]), 2.0 * pkg.ldiv(F, B[:, 0]) - 3.0 * pkg.ldiv(F, B[:, 1])) < 1e-10
    # L^-T z has covariance A^-1:  z^T z == x^T A x for x = L^-T z
    Z = rng.standard_normal((w.n, 2))
    Xs = pkg.backward_solve(F, Z)
    assert np.allclose(np.sum(Xs * (w.Q @ Xs), axis=0), np.sum(Z * Z, axis=0), rtol=1e-9)
    ld = F.logdet()
    F.refactor(4.0 * w.Q.data)
    assert abs(F.logdet() - (ld + w.n * np.log(4.0))) < 1e-9 * abs(ld)


def test_full_size_properties_elliptic512(pkg):
    """BASELINE config[3] at full size (512 x 512 nodes, 256 blocks of 1024, 6.4 GB of factor):
    size-independent properties; 256 device-Philox samples split as two ranks would draw them."""
    w = pkg.workloads.make("elliptic512")
    F = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
    mu = pkg.ldiv(F, w.rhs)
    qn = abs(w.Q).sum(axis=1).max()
    assert np.linalg.norm(w.Q @ mu - w.rhs) / (qn * np.linalg.norm(mu) + np.linalg.norm(w.rhs)) < 1e-14
    rng = np.random.default_rng(1)
    Z = rng.standard_normal((w.n, 2))
    Xs = pkg.backward_solve(F, Z)
    assert np.allclose(np.sum(Xs * (w.Q @ Xs), axis=0), np.sum(Z * Z, axis=0), rtol=1e-9)
    B = rng.standard_normal((w.n, 2))
    assert rel(pkg.backward_solve(F, pkg.forward_solve(F, B)), pkg.ldiv(F, B)) < 1e-13
    # sample ids 128..255 drawn alone equal the second half of one 256-sample call (rank invariance)
    Xa = F.sample(256, mean=mu, seed=9)
    Xb = F.sample(128, mean=mu, seed=9, first_id=128)
    assert np.array_equal(Xa[:, 128:], Xb)


def test_batch_of_problems_matches_one_by_one(pkg):
    """B independent problems on one pattern, factored / solved / sampled in lock step, equal the same
    problems handled one at a time through the same launch sequence (set_eager bit 1: tile / panel /
    update steps and doubling also for one problem) bitwise -- same kernels, same order of operations --
    and the default one-problem path (fused look-ahead steps, inverse rows) to rounding."""
    w = pkg.workloads.make("darcy32")
    B, k = 3, 16
    rng = np.random.default_rng(4)
    vals = np.stack([w.Q.data * (1.0 + 0.3 * p) for p in range(B)])
    rhs = np.stack([w.rhs * (p + 1.0) for p in range(B)])
    Fb = pkg.TridiagonalCholeskyFactor(batch=B).factor(w.Q, w.n_blocks, values=vals)
    mu_b = Fb.solve_batch(rhs[:, None, :])[:, 0, :]
    X_b = Fb.sample_batch(k, mean=mu_b, seed=11, first_id=100)
    Bm = rng.standard_normal((B, k, w.n))
    Y_b = Fb.solve_batch(Bm, pkg._cabi.SOLVE_BACKWARD)
    for p in range(B):
        Qp = w.Q.copy(); Qp.data = vals[p]
        F1 = pkg.TridiagonalCholeskyFactor()
        F1.set_eager(Switch.BATCH_ROUTES)
        F1.factor(Qp, w.n_blocks)
        mu1 = pkg.ldiv(F1, rhs[p])
        assert np.array_equal(mu_b[p], mu1)
        assert rel(pkg.ldiv(pkg.tridiagonal_cholesky(Qp, w.n_blocks), rhs[p]), mu1) < solve_tol(w)
        X1 = F1.sample(k, mean=mu1, seed=11, first_id=100 + p * k)
        assert np.array_equal(X_b[p].T, X1)
        assert np.array_equal(Y_b[p].T, pkg.backward_solve(F1, Bm[p].T))
        Fb.select_problem(p)
        assert np.array_equal(Fb.chos[2], F1.chos[2]) and abs(Fb.logdet() - F1.logdet()) == 0.0
        Fo = O.tridiagonal_cholesky(Qp, w.n_blocks)
        assert rel(mu_b[p], O.ldiv(Fo, rhs[p])) < solve_tol(w)
    # exact marginal variances of the whole batch in one call
    vb = Fb.marginal_var("exact")
    assert vb.shape == (B, w.n)
    for p in (0, B - 1):
        Qp = w.Q.copy(); Qp.data = vals[p]
        vo = O.marginal_variances_exact(O.tridiagonal_cholesky(Qp, w.n_blocks))
        assert np.max(np.abs(vb[p] - vo) / vo) < 1e-9
    # sampled variances of the whole batch: RBMCStrategy(k) per problem, problem 0 = the one-problem path
    Qc = pkg.CsrMatrix(w.Q)
    vr = Fb.marginal_var("rbmc", k=64, seed=9, Q=Qc, q_values=vals)
    vm = Fb.marginal_var("mc", k=64, seed=9)
    Q0 = w.Q.copy(); Q0.data = vals[0]
    F0 = pkg.TridiagonalCholeskyFactor()
    F0.set_eager(Switch.BATCH_ROUTES)
    F0.factor(Q0, w.n_blocks)
    assert np.array_equal(vr[0], F0.marginal_var("rbmc", k=64, seed=9, Q=pkg.CsrMatrix(Q0)))
    assert np.array_equal(vm[0], F0.marginal_var("mc", k=64, seed=9))
    for p in range(B):
        Qp = w.Q.copy(); Qp.data = vals[p]
        vo = O.marginal_variances_exact(O.tridiagonal_cholesky(Qp, w.n_blocks))
        assert np.median(np.abs(vr[p] - vo) / vo) < 0.12 and np.median(np.abs(vm[p] - vo) / vo) < 0.25   # k = 64 samples
    # a non-SPD member of the batch is reported with its block index
    bad = vals.copy()
    Qb = w.Q.tocsc()
    d = np.flatnonzero((Qb.indices == 700) & (np.repeat(np.arange(w.n), np.diff(Qb.indptr)) == 700))[0]
    bad[1, d] = -1e20
    with pytest.raises(pkg.NotPositiveDefinite) as e:
        Fb.refactor(bad)
    assert e.value.info == 700 // w.block_size + 1


def test_config_burgers512x64_against_oracle(pkg):
    """BASELINE config[0] at full size (n = 32768, 64 temporal blocks of 512): posterior mean
    against the oracle, plus residual."""
    w = pkg.workloads.make("burgers512x64")
    F = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
    Fo = O.tridiagonal_cholesky(w.Q, w.n_blocks)
    mu = pkg.ldiv(F, w.rhs)
    assert rel(mu, O.ldiv(Fo, w.rhs)) < solve_tol(w)
    qn = abs(w.Q).sum(axis=1).max()
    assert np.linalg.norm(w.Q @ mu - w.rhs) / (qn * np.linalg.norm(mu) + np.linalg.norm(w.rhs)) < 1e-14
    assert np.max(np.abs(np.tril(F.chos[63]) - Fo.chos[63])) / np.max(np.abs(Fo.chos[63])) < TOL_FACTOR
    assert abs(F.logdet() - O.logdet(Fo)) < 1e-10 * abs(O.logdet(Fo))


def test_two_level_panel_factor_of_batches(pkg):
    """Batches factor a block in 128-column diagonal blocks (potrf_diag128) with GEMM panels and rank-256 trailing updates.
    burgers512x64 (8 tiles per block) as a batch of two: against the oracle, and bitwise against a
    single problem driven through the same three-launch / two-level path (set_eager bit 1)."""
    w = pkg.workloads.make("burgers512x64")
    vals = np.stack([w.Q.data, w.Q.data * 1.25])
    rhs = np.stack([w.rhs, w.rhs * 2.0])
    Fb = pkg.TridiagonalCholeskyFactor(batch=2).factor(w.Q, w.n_blocks, values=vals)
    mu_b = Fb.solve_batch(rhs[:, None, :])[:, 0, :]
    Fo = O.tridiagonal_cholesky(w.Q, w.n_blocks)
    assert rel(mu_b[0], O.ldiv(Fo, w.rhs)) < solve_tol(w)
    assert rel(mu_b[1], O.ldiv(Fo, w.rhs) * (2.0 / 1.25)) < solve_tol(w)
    qn = abs(w.Q).sum(axis=1).max()
    assert np.linalg.norm(w.Q @ mu_b[0] - w.rhs) / (qn * np.linalg.norm(mu_b[0]) + np.linalg.norm(w.rhs)) < 1e-14
    Fb.select_problem(0)
    assert np.max(np.abs(np.tril(Fb.chos[63]) - Fo.chos[63])) / np.max(np.abs(Fo.chos[63])) < TOL_FACTOR
    assert abs(Fb.logdet() - O.logdet(Fo)) < 1e-10 * abs(O.logdet(Fo))
    F1 = pkg.TridiagonalCholeskyFactor()
    F1.set_eager(Switch.BATCH_ROUTES)
    F1.factor(w.Q, w.n_blocks)
    assert np.array_equal(F1.chos[63], Fb.chos[63]) and np.array_equal(pkg.ldiv(F1, w.rhs), mu_b[0])
    F1.set_eager(0)                      # fused one-launch step: same factor up to rounding
    F1.refactor(w.Q.data)
    assert 0 < np.max(np.abs(F1.chos[63] - Fb.chos[63])) / np.max(np.abs(Fo.chos[63])) < 1e-12
    # round 4: a batch this small (7 workgroups per problem fit the chip) factors the 256 x 256 diagonal block of every panel in
    # ONE persistent launch (potrf_persist on the block's 4 x 4 tiles) instead of two potrf_diag128 launches and four 128^3
    # GEMMs; set_eager bit 15 keeps those.  Same factor and inverse up to rounding, same oracle tolerance; each route launches its
    # own kernels and none of the other's (round 5: the persistent launches are kernel class 17 of the statistics -- the rocprof
    # symbol potrf_persist -- and the route is in gmrf_stats.persist_route; the one-workgroup potrf_panel256 of round 4 is gone)
    is128 = lambda F: any(s["M"] == 128 and s["N"] == 128 and s["K"] == 128 for s in F.gemm_shapes())
    Fb.set_profiling(1); Fb.refactor(vals); st = Fb.stats(); Fb.set_profiling(0)
    assert st["kernel_launches"][16] == 0 and st["kernel_launches"][17] == (w.block_size // 256) * w.n_blocks and not is128(Fb)
    assert st["persist_route"] == 3 and st["persist_cus"] == 14 and st["persist_refused"] == 0 and st["persist_aborts"] == 0
    Fd = pkg.TridiagonalCholeskyFactor(batch=2)
    Fd.set_eager(Switch.NO_PERSIST_PANELS)
    Fd.factor(w.Q, w.n_blocks, values=vals)
    Fd.select_problem(0)
    assert 0 < np.max(np.abs(Fd.chos[63] - Fb.chos[63])) / np.max(np.abs(Fo.chos[63])) < 1e-12
    Xd, Xb = Fd.get_block(pkg._cabi.BLOCK_LINV, 31), Fb.get_block(pkg._cabi.BLOCK_LINV, 31)
    assert np.max(np.abs(Xd - Xb)) < 1e-11 * np.max(np.abs(Xb))
    assert rel(Fd.solve_batch(rhs[:, None, :])[0, 0], mu_b[0]) < solve_tol(w)      # (two roundings of one ill-conditioned solve)
    Fd.set_profiling(1); Fd.refactor(vals); std = Fd.stats(); Fd.set_profiling(0)
    assert std["kernel_launches"][16] == 2 * (w.block_size // 256) * w.n_blocks and std["kernel_launches"][17] == 0 and is128(Fd)
    assert std["persist_route"] == 0 and std["persist_cus"] == 0


def test_config_elliptic_long_chain_properties(pkg):
    """BASELINE config[3] family (elliptic, bs = 2 node rows) with a long chain: 128 x 128 nodes ->
    64 blocks of 256; size-independent properties and the oracle."""
    w = pkg.workloads.elliptic(128)
    F = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
    Fo = O.tridiagonal_cholesky(w.Q, w.n_blocks)
    B = np.random.default_rng(1).standard_normal((w.n, 32))
    assert rel(pkg.ldiv(F, B), O.ldiv(Fo, B)) < solve_tol(w)
    X = pkg.backward_solve(F, B)
    assert np.allclose(np.sum(X * (w.Q @ X), axis=0), np.sum(B * B, axis=0), rtol=1e-9)


def test_large_block_size_4096(pkg):
    """Block size of BASELINE config[4] (bs = 4096, 64 tiles per block, six doubling levels of the
    block inverse) on a short, well-conditioned chain."""
    w = pkg.workloads.random_block_tridiagonal(3, 4096, seed=8, density=0.002)
    F = pkg.tridiagonal_cholesky(w.Q, 3)
    mu = pkg.ldiv(F, w.rhs)
    qn = abs(w.Q).sum(axis=1).max()
    assert np.linalg.norm(w.Q @ mu - w.rhs) / (qn * np.linalg.norm(mu) + np.linalg.norm(w.rhs)) < 1e-14
    import scipy.sparse.linalg as spla
    assert rel(mu, spla.splu(w.Q.tocsc()).solve(w.rhs)) < 1e-12


def test_posterior_assembly_and_gauss_newton_on_device(pkg):
    """A = Q + noise J'J and rhs = Qx_prior + noise J'(J x + obs_diff)
    (scripts/solve_burger.jl:143-149) assembled on the device from values only, re-factored on the
    analysed pattern, three Gauss-Newton iterations against the oracle."""
    import torch
    gn = pkg.workloads.burgers_gauss_newton(64, 8)
    x = gn["x_prior"].copy()
    J = gn["jacobian"](x)
    asm = pkg.PosteriorAssembler(gn["Q"], J)
    noise = gn["noise"]
    # values against SciPy, entry by entry (same pattern, fixed summation order)
    a = asm.precision(gn["Q"].data, J.data, noise)
    A = O.assemble_posterior(gn["Q"], J, noise)
    assert np.max(np.abs(a - A.data)) / np.max(np.abs(A.data)) < 1e-15
    r = gn["residual"](x)
    rhs = asm.rhs(gn["Qx_prior"], J.data, x, -r, noise)
    rhs_o = O.gn_rhs(gn["Qx_prior"], J, x, -r, noise)
    assert np.linalg.norm(rhs - rhs_o) / np.linalg.norm(rhs_o) < 1e-14
    # device-resident loop: only J's values and the residual cross the bus per iteration
    P = asm.pattern.copy(); P.data = a
    F = pkg.tridiagonal_cholesky(P, gn["n_blocks"])
    qd = torch.from_numpy(gn["Q"].data).cuda(); qx = torch.from_numpy(gn["Qx_prior"]).cuda()
    xo = x.copy()
    for it in range(3):
        J = gn["jacobian"](xo)
        r = gn["residual"](xo)
        x_dev = pkg.gn_step(F, asm, qd, qx, torch.from_numpy(J.data).cuda(), torch.from_numpy(xo).cuda(),
                            torch.from_numpy(-r).cuda(), noise)
        x_ora = O.gn_step(gn["Q"], J, gn["Qx_prior"], xo, -r, noise, gn["n_blocks"])
        assert x_dev.is_cuda
        assert rel(x_dev.cpu().numpy(), x_ora) < 1e-9
        xo = x_ora


def test_condition_on_observations_problem_loop(pkg):
    """The reference's Darcy problem loop (scripts/darcy/solve_darcy_gmrf-fem.jl:176-192) through the
    Python twin of `condition_on_observations`: condition, mean, std, rand; then the next coefficient
    field with values only (same pattern)."""
    Q0, obs, N = pkg.workloads.darcy_conditioning(32, seeds=(523802340, 11))
    (A, y), (A2, y2) = obs
    x = pkg.condition_on_observations(Q0, None, A, 1e8, y, N)
    Qp, Fo, mu_o = O.condition_on_observations(Q0, None, A, 1e8, y, N)
    w = pkg.workloads.make("darcy32")                  # same posterior as the packaged workload
    assert abs(x.precision_matrix() - Qp).max() / abs(Qp).max() < 1e-15
    assert rel(x.mean(), mu_o) < solve_tol(w)
    vo = O.marginal_variances_exact(Fo)
    assert np.max(np.abs(x.std() - np.sqrt(vo)) / np.sqrt(vo)) < 1e-9
    assert abs(x.logdet() - O.logdet(Fo)) < 1e-10 * abs(O.logdet(Fo))
    s_rb = x.std("rbmc", k=50, seed=3)                 # RBMCStrategy(50) of the reference
    assert np.median(np.abs(s_rb - np.sqrt(vo)) / np.sqrt(vo)) < 0.05
    X = x.rand(8, seed=5)
    Z = x.F.normals(8, seed=5)
    assert rel(X, O.sample(Fo, mu_o, Z)) < solve_tol(w)
    # sqmahal / nll of a field under the conditioned GMRF (scripts/burgers/solve_burgers_gmrf-collocation.jl:208-215, :262)
    zt = mu_o + 0.1 * np.random.default_rng(9).standard_normal(mu_o.size)
    dz = zt - mu_o
    sq_o = float(dz @ (Qp @ dz))
    assert abs(x.sqmahal(zt) - sq_o) < 1e-9 * sq_o          # (the device mean differs from the oracle's by solve_tol)
    nll_o = 0.5 * (mu_o.size * np.log(2.0 * np.pi) + sq_o - O.logdet(Fo))
    assert abs(x.nll(zt) - nll_o) < 1e-9 * abs(nll_o)
    # next problem: new coefficient field, same pattern -> values only
    x.update(A2.data, y2)
    Qp2, Fo2, mu2 = O.condition_on_observations(Q0, None, A2, 1e8, y2, N)
    assert rel(x.mean(), mu2) < solve_tol(w)
    assert np.max(np.abs(x.var() - O.marginal_variances_exact(Fo2)) / O.marginal_variances_exact(Fo2)) < 1e-9


# ----------------------------------------------------------------------------- round 2: parity at the BASELINE sizes

def _hip_memcpy_d2d(dst_ptr, src_ptr, nbytes):
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(C.c_void_p(dst_ptr), C.c_void_p(src_ptr), C.c_size_t(nbytes), 3) == 0


def test_config_darcy256_against_oracle(pkg):
    """BASELINE metric config (C3: 256 x 256 Darcy, 64 blocks of 1024) against the oracle at FULL size:
    posterior mean, 64 samples with given z, log-determinant, exact marginal variances of the last
    eight blocks, factor blocks.  Tolerance: 0.25 * cond(Q) * eps (cond = 3.4e9 -> 1.9e-7), justified by
    test_forward_error_not_worse_than_lapack; variances max(1e-9, 0.01 * cond * eps) = 7.5e-9 relative
    (BASELINE.md's flat 1e-9 holds up to cond ~ 4e8; measured here 1.4e-9 on variances of 1.3e-11)."""
    w = pkg.workloads.make("darcy256")
    w.meta.setdefault("cond", 3.4e9)               # measured once (tools/accuracy_check.py); eigsh at n = 65536 takes minutes
    F = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
    Fo = O.tridiagonal_cholesky(w.Q, w.n_blocks)
    tol = solve_tol(w)
    mu, mu_o = pkg.ldiv(F, w.rhs), O.ldiv(Fo, w.rhs)
    assert rel(mu, mu_o) < tol
    Z = np.random.default_rng(7).standard_normal((w.n, 64))
    assert rel(F.sample(64, mean=mu_o, z=Z), O.sample(Fo, mu_o, Z)) < tol
    assert abs(F.logdet() - O.logdet(Fo)) < 1e-10 * abs(O.logdet(Fo))
    for i in (0, 31, 63):
        assert np.max(np.abs(np.tril(F.chos[i]) - Fo.chos[i])) / np.max(np.abs(Fo.chos[i])) < TOL_FACTOR
    for i in (0, 62):
        assert np.max(np.abs(F.Cs[i] - Fo.Cs[i])) / np.max(np.abs(Fo.Cs[i])) < TOL_FACTOR
    vo = O.marginal_variances_exact(Fo, last_blocks=8)
    v = F.marginal_var("exact")[-vo.size:]
    assert np.max(np.abs(v - vo) / vo) < max(1e-9, 0.01 * w.meta["cond"] * EPS)


@pytest.mark.parametrize("name", ["burgers512x64", "darcy64", "darcy256"])
def test_forward_error_not_worse_than_lapack(pkg, name):
    """Why the parity gate is cond-aware: against an extended-precision solution (iterative refinement
    with long-double residuals) the HIP path is as close to the truth as the LAPACK-backed oracle --
    both sit at O(cond * eps), so the two cannot agree with each other any better.  Asserted: HIP
    forward error <= 3 x the oracle's, on BASELINE configs C1, C2, C3.  (2 x until round 4; the round-5 tile Cholesky groups its
    sums differently -- one subtraction per panel owner instead of one per panel -- and darcy64 came out at 1.7e-11 against the
    oracle's 7.7e-12 with cond * eps = 1.4e-9: both two orders below what the conditioning allows, neither systematically the
    better one.)"""
    w = pkg.workloads.make(name)
    Fo = O.tridiagonal_cholesky(w.Q, w.n_blocks)
    x_o = O.ldiv(Fo, w.rhs)
    Ql = w.Q.tocsr().astype(np.longdouble)
    bl = w.rhs.astype(np.longdouble)
    x = x_o.astype(np.longdouble)
    for _ in range(6):
        x = x + O.ldiv(Fo, np.asarray(bl - Ql @ x, dtype=np.float64)).astype(np.longdouble)
    x_true = np.asarray(x, dtype=np.float64)
    F = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
    x_g = pkg.ldiv(F, w.rhs)
    err_o, err_g = rel(x_o, x_true), rel(x_g, x_true)
    print(f"{name}: forward error oracle {err_o:.2e}, HIP {err_g:.2e}, HIP vs oracle {rel(x_g, x_o):.2e}")
    assert err_g <= 3.0 * err_o + 1e-15
    assert rel(x_g, x_o) <= 3.0 * max(err_o, err_g) + 1e-15


def test_config_burgers4096x512_full_size(pkg):
    """BASELINE config[4] (C5) at FULL size: 4096 spatial nodes x 512 time steps, n = 2 097 152, 512
    blocks of 4096, fp32-value SpMV / SpMM with fp64 accumulation.  (i) size-independent properties of
    the full chain: backward error, backward o forward = ldiv, z'z = x'Ax; (ii) the oracle on a
    truncated chain (4096 x 4 blocks); (iii) SpMV / SpMM on the 31 M-entry precision matrix, fp64 and
    fp32 values, against SciPy."""
    import torch
    w = pkg.workloads.make("burgers4096x512")
    assert (w.n, w.n_blocks, w.block_size) == (2097152, 512, 4096)
    F = pkg.TridiagonalCholeskyFactor()
    F.set_keep_l(False)                              # 137 GB of factor instead of 206 GB
    F.factor(w.Q, w.n_blocks)
    mu = pkg.ldiv(F, w.rhs)
    qn = abs(w.Q).sum(axis=1).max()
    assert np.linalg.norm(w.Q @ mu - w.rhs) / (qn * np.linalg.norm(mu) + np.linalg.norm(w.rhs)) < 1e-14
    rng = np.random.default_rng(5)
    B = rng.standard_normal((w.n, 2))
    assert rel(pkg.backward_solve(F, pkg.forward_solve(F, B)), pkg.ldiv(F, B)) < 1e-13
    Xs = pkg.backward_solve(F, B)
    assert np.allclose(np.sum(Xs * (w.Q @ Xs), axis=0), np.sum(B * B, axis=0), rtol=1e-9)
    with pytest.raises(pkg.GmrfError):               # the L blocks were not kept
        F.get_block(pkg._cabi.BLOCK_L, 0)
    ld_full = F.logdet()
    assert np.isfinite(ld_full)
    F.close()
    # (iii) K6 on the full precision matrix
    Qr = w.Q.tocsr()
    X = rng.standard_normal((w.n, 8))
    S64, S32 = pkg.CsrMatrix(Qr), pkg.CsrMatrix(Qr, values_f32=True)
    Q32 = Qr.copy(); Q32.data = Q32.data.astype(np.float32).astype(np.float64)
    ref64, ref32 = Qr @ X, Q32 @ X
    assert rel(S64 @ X, ref64) < 1e-14 and rel(S64 @ X[:, 0], ref64[:, 0]) < 1e-14
    assert rel(S32 @ X, ref32) < 1e-14 and rel(S32 @ X[:, 0], ref32[:, 0]) < 1e-14
    assert rel(S32 @ X, ref64) < 1e-6                # fp32 values: 2^-24 relative per entry, fp64 accumulation
    X64h = np.tile(X, (1, 8))                                         # 64 right-hand sides, device resident
    Xc = torch.from_numpy(np.ascontiguousarray(X64h.T)).cuda().t()   # column-major (each right-hand side contiguous)
    Yc = (S32 @ Xc).cpu().numpy()
    assert rel(Yc[:, :8], ref32) < 1e-14 and np.array_equal(Yc[:, 56:], Yc[:, :8])
    Yr = (S32 @ torch.from_numpy(X64h).cuda()).cpu().numpy()         # node-major: the LDS-tiled kernel
    assert rel(Yr[:, :8], ref32) < 1e-14 and np.array_equal(Yr[:, 56:], Yr[:, :8])
    del S64, S32
    # (ii) the same model with 4 time steps against the oracle (bs = 4096: two-level panels, six doubling levels)
    wt = pkg.workloads.burgers(4096, 4)
    Ft = pkg.tridiagonal_cholesky(wt.Q, wt.n_blocks)
    Fo = O.tridiagonal_cholesky(wt.Q, wt.n_blocks)
    # two backward-stable factorisations of an ill-conditioned 4096 x 4096 block agree to cond * eps, not to
    # 1e-11 (measured 9.5e-10 of max|L|): the blocks are held to the solve tolerance, and block 0 to the
    # backward-error bound  || L L' - D || <= c n eps || D ||  that both must meet
    ftol = max(TOL_FACTOR, solve_tol(wt))
    for i in (0, 3):
        assert np.max(np.abs(np.tril(Ft.chos[i]) - Fo.chos[i])) / np.max(np.abs(Fo.chos[i])) < ftol
    assert np.max(np.abs(Ft.Cs[2] - Fo.Cs[2])) / np.max(np.abs(Fo.Cs[2])) < ftol
    D0 = wt.Q.tocsr()[:4096, :4096].toarray()
    L0 = np.tril(Ft.chos[0])
    assert np.linalg.norm(L0 @ L0.T - D0) / np.linalg.norm(D0) < 4096 * EPS
    Bt = rng.standard_normal((wt.n, 3))
    xo = O.ldiv(Fo, Bt)
    assert rel(pkg.ldiv(Ft, Bt), xo) < solve_tol(wt)
    assert abs(Ft.logdet() - O.logdet(Fo)) < 1e-10 * abs(O.logdet(Fo))


def test_staircase_of_the_coupling_blocks_is_exact(pkg):
    """The symbolic phase finds, per 64-row tile, the first non-zero column of the coupling blocks;
    G2 (S = D - C C^T), the C products of the sweeps and the sparse C = B X^T skip what lies left of
    it.  Skipped terms are exact zeros: the factor is BITWISE the one the dense window gives
    (set_eager bit 5), solves agree to rounding (the k = 1 kernels deal the row to lanes differently)."""
    for name in ("darcy64", "elliptic32", "burgers64x8"):
        w = pkg.workloads.make(name)
        Fs = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
        Fd = pkg.TridiagonalCholeskyFactor()
        Fd.set_eager(Switch.NO_STAIRCASE)
        Fd.factor(w.Q, w.n_blocks)
        lay_s, lay_d = Fs.get_layout(), Fd.get_layout()
        # record = [cmin, rmax, row tiles, kst..., split of the inverses (0 here: one problem)]
        assert tuple(lay_s[:3]) == tuple(lay_d[:3]) and np.all(lay_d[3:] == 0) and np.all(np.diff(lay_s[3:-1]) >= 0) and lay_s[-1] == 0
        if name == "darcy64":                       # 4 node rows of 64 per block, reach 3 rows: tile a starts at column 64 (a + 1)
            assert list(lay_s) == [64, 192, 3, 0, 64, 128, 0]
        for i in (0, w.n_blocks // 2, w.n_blocks - 1):
            assert np.array_equal(Fs.chos[i], Fd.chos[i])
            assert np.array_equal(Fs.get_block(pkg._cabi.BLOCK_LINV, i), Fd.get_block(pkg._cabi.BLOCK_LINV, i))
            if i < w.n_blocks - 1:
                assert np.array_equal(Fs.Cs[i], Fd.Cs[i])
        B = np.random.default_rng(2).standard_normal((w.n, 64))
        for b in (w.rhs, B[:, :3], B):
            assert rel(pkg.ldiv(Fs, b), pkg.ldiv(Fd, b)) < 1e-13
        assert np.max(np.abs(Fs.marginal_var("exact") / Fd.marginal_var("exact") - 1.0)) < 1e-12
    # a batch takes the GEMM route for 64 right-hand sides: staircase bounds per tile of the GEMM
    w = pkg.workloads.make("darcy64")
    vals = np.tile(w.Q.data, (32, 1))
    Fb = pkg.TridiagonalCholeskyFactor(batch=32).factor(w.Q, w.n_blocks, values=vals)
    Bm = np.random.default_rng(3).standard_normal((32, 64, w.n))
    Fo = O.tridiagonal_cholesky(w.Q, w.n_blocks)
    for mode, fo in ((pkg._cabi.SOLVE_FULL, O.ldiv), (pkg._cabi.SOLVE_FORWARD, O.forward_solve), (pkg._cabi.SOLVE_BACKWARD, O.backward_solve)):
        Y = Fb.solve_batch(Bm, mode)
        assert rel(Y[5].T, fo(Fo, Bm[5].T)) < solve_tol(w)


def test_without_the_l_blocks(pkg):
    """gmrf_bt_set_keep_l(h, 0): the triangular blocks live in a one-block work buffer; solves, samples,
    variances and the log-determinant are bitwise those of a handle that keeps them; F.chos raises."""
    w = pkg.workloads.make("darcy64")
    F1 = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
    F0 = pkg.TridiagonalCholeskyFactor()
    F0.set_keep_l(False)
    F0.factor(w.Q, w.n_blocks)
    assert np.array_equal(pkg.ldiv(F0, w.rhs), pkg.ldiv(F1, w.rhs))
    assert np.array_equal(F0.sample(8, seed=3), F1.sample(8, seed=3))
    assert np.array_equal(F0.marginal_var("exact"), F1.marginal_var("exact"))
    assert F0.logdet() == F1.logdet()
    assert np.array_equal(F0.Cs[3], F1.Cs[3])
    with pytest.raises(pkg.GmrfError) as e:
        F0.chos[0]
    assert e.value.status == pkg._cabi.ERR_NO_FACTOR
    with pytest.raises(pkg.GmrfError):
        F0.export_factor()
    bs = w.n // w.n_blocks                                # exactly the N triangular blocks are gone
    assert F1.stats()["factor_bytes"] - F0.stats()["factor_bytes"] == 8 * bs * bs * w.n_blocks
    assert F0.stats()["factor_bytes"] < 0.65 * F1.stats()["factor_bytes"]
    # a batch, re-factored with new values
    vals = np.stack([w.Q.data, 2.0 * w.Q.data])
    Fb = pkg.TridiagonalCholeskyFactor(batch=2)
    Fb.set_keep_l(False)
    Fb.factor(w.Q, w.n_blocks, values=vals)
    Fb.select_problem(1)
    assert abs(Fb.logdet() - (F1.logdet() + w.n * np.log(2.0))) < 1e-10 * abs(F1.logdet())
    F0.set_keep_l(True)                               # back: the next factorisation keeps them again
    F0.factor(w.Q, w.n_blocks)
    assert np.array_equal(F0.chos[2], F1.chos[2])


def test_external_storage_with_a_batch_and_refresh(pkg, lib):
    """Caller-owned factor storage (torch tensors) for a BATCH of problems: sizes scale with the batch
    (gmrf_bt_storage_bytes), a mismatching batch is refused, nothing is written past the buffers
    (guard words), and attaching storage drops whatever the handle had factored."""
    import ctypes as C
    import torch
    w = pkg.workloads.make("darcy32")
    B = 3
    vals = np.stack([w.Q.data * (1.0 + p) for p in range(B)])
    rhs = np.stack([w.rhs] * B)
    F = pkg.TridiagonalCholeskyFactor(batch=B)
    F.factor(w.Q, w.n_blocks, values=vals)
    ref = F.solve_batch(rhs[:, None, :])
    bl, bc, bi = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    pkg._cabi.check(lib.gmrf_bt_storage_bytes(w.n, w.n_blocks, B, C.byref(bl), C.byref(bc), C.byref(bi)))
    guard = 1024
    bufs = [torch.full((b.value // 8 + guard,), 777.0, dtype=torch.float64, device="cuda") for b in (bl, bc, bi)]
    assert lib.gmrf_bt_set_storage(F._h, w.n, w.n_blocks, 1, *[pkg._cabi.ptr(b) for b in bufs]) == pkg._cabi.ERR_BAD_SHAPE
    pkg._cabi.check(lib.gmrf_bt_set_storage(F._h, w.n, w.n_blocks, B, *[pkg._cabi.ptr(b) for b in bufs]))
    with pytest.raises(pkg.GmrfError) as e:           # the old factor is gone with the old buffers
        F.solve_batch(rhs[:, None, :])
    assert e.value.status == pkg._cabi.ERR_NO_FACTOR
    F.factor(w.Q, w.n_blocks, values=vals)
    assert np.array_equal(F.solve_batch(rhs[:, None, :]), ref)
    for b in bufs:
        assert bool((b[-guard:] == 777.0).all())
    F.select_problem(2)
    Fo = O.tridiagonal_cholesky(w.Q, w.n_blocks)
    assert np.max(np.abs(np.tril(F.chos[1]) - np.sqrt(3.0) * Fo.chos[1])) / np.max(np.abs(Fo.chos[1])) < 1e-11


def test_factor_moves_between_handles_with_its_layout(pkg):
    """What a rank that receives the factor by broadcast does: adopt the root's layout record, fill the
    Linv and C buffers (device copies here), commit -- into a handle that had analysed a DIFFERENT
    coupling pattern before.  And the import of a factor image into such a handle."""
    wa = pkg.workloads.make("darcy32")                             # stencil coupling: window + staircase
    wb = pkg.workloads.random_block_tridiagonal(wa.n_blocks, wa.block_size, seed=5, density=0.05)   # scattered coupling: dense window
    assert wb.n == wa.n
    Fa = pkg.tridiagonal_cholesky(wa.Q, wa.n_blocks)               # analysed pattern a ...
    Fb = pkg.tridiagonal_cholesky(wb.Q, wb.n_blocks)
    xb = pkg.ldiv(Fb, wb.rhs)
    assert not np.array_equal(Fa.get_layout(), Fb.get_layout())    # (same window at this size, other staircase)
    # ... then receives factor b: layout, buffers, commit
    Fa.adopt_layout(wb.n, wb.n_blocks, Fb.get_layout())
    for kind in (pkg._cabi.BLOCK_LINV, pkg._cabi.BLOCK_C):
        (src, nb), (dst, nd) = Fb.factor_buffer(kind), Fa.factor_buffer(kind)
        assert nb == nd
        _hip_memcpy_d2d(dst, src, nb)
    Fa.adopt_commit(False)
    assert np.array_equal(pkg.ldiv(Fa, wb.rhs), xb)
    assert np.array_equal(Fa.sample(4, seed=2), Fb.sample(4, seed=2))
    assert np.array_equal(Fa.marginal_var("exact"), Fb.marginal_var("exact"))     # sweeps and variances see the same C
    with pytest.raises(pkg.GmrfError):
        Fa.chos[0]                                                  # the L blocks did not travel
    with pytest.raises(pkg.GmrfError):
        Fa.refactor(wa.Q.data)                                      # pattern a no longer describes this handle
    # import of a dense image into a handle that analysed pattern a (window + staircase)
    Fc = pkg.tridiagonal_cholesky(wa.Q, wa.n_blocks)
    Fc.import_factor(Fb.export_factor())
    assert np.array_equal(pkg.ldiv(Fc, wb.rhs), xb)
    assert np.array_equal(Fc.marginal_var("exact"), Fb.marginal_var("exact"))
    assert list(Fc.get_layout()[:2]) == [0, 64 * ((wb.block_size + 63) // 64)]
    Fc.factor(wa.Q, wa.n_blocks)                                    # and back to its own pattern
    assert np.array_equal(pkg.ldiv(Fc, wa.rhs), pkg.ldiv(pkg.tridiagonal_cholesky(wa.Q, wa.n_blocks), wa.rhs))


def test_spmm_node_major_lds_tiles(pkg):
    """K6 with node-major right-hand sides (the k values of a node contiguous): the LDS-tiled kernel
    (tile plan: distinct columns per 64-row tile, 16-bit local indices; X rows staged in LDS once per
    tile) for even k, the plain node-major kernel for odd k and for tiles beyond the LDS image;
    fp64 and fp32 values; against SciPy and against the column-major kernel."""
    import torch
    w = pkg.workloads.make("darcy64")
    Qr = w.Q.tocsr()
    S64, S32 = pkg.CsrMatrix(Qr), pkg.CsrMatrix(Qr, values_f32=True)
    Q32 = Qr.copy(); Q32.data = Q32.data.astype(np.float32).astype(np.float64)
    rng = np.random.default_rng(4)
    for k in (2, 16, 50, 64, 70, 5):
        X = rng.standard_normal((w.n, k))                       # C-contiguous = node-major
        assert rel(S64 @ X, Qr @ X) < 1e-14
        assert rel(S32 @ X, Q32 @ X) < 1e-14
        Xd = torch.from_numpy(X).cuda()
        Yd = S64 @ Xd
        assert Yd.is_cuda and Yd.shape == (w.n, k) and np.array_equal(Yd.cpu().numpy(), S64 @ X)
        assert rel(S64 @ np.asfortranarray(X), Qr @ X) < 1e-14   # column-major operand: the lane-group kernel
    # every right-hand side of the tiled kernel sums its row in entry order: a column does not depend on its neighbours
    X = rng.standard_normal((w.n, 16))
    Y = S64 @ X
    assert np.array_equal(Y[:, 3], (S64 @ np.ascontiguousarray(X[:, 2:6]))[:, 1])
    assert rel(Y[:, 3], S64 @ np.ascontiguousarray(X[:, 3])) < 1e-15
    # ragged: empty rows, a row count that is no multiple of the tile, rectangular, 64-row tiles with too many distinct
    # columns (the plan settles for 32-row tiles of up to 224: the padded kernel with 7 gather loads, NOT the plain kernel);
    # a dense-ish matrix whose 16-row tiles are beyond the LDS image (no plan: the plain node-major kernel)
    def last_rows_route(S):
        out = np.zeros(12, np.int64)
        pkg._cabi.check(pkg._cabi.load().gmrf_test_spmm_route(S._h, pkg._cabi.ptr(np.array([2, 2, 2, 0, 0, 0, 0, 0], np.int64)), None, None,
                                                              pkg._cabi.ptr(out)))
        return tuple(int(v) for v in (out[9], out[10], out[1]))          # kind (0 plain, 1 tiled, 2 padded), NG, tile height
    A = sp.random(1000, 700, density=0.01, random_state=rng, data_rvs=rng.standard_normal).tolil()
    A[5, :] = 0.0; A[999, :] = 0.0
    A = A.tocsr(); A.eliminate_zeros()
    Xa = rng.standard_normal((700, 8))
    Sa = pkg.CsrMatrix(A)
    assert rel(Sa @ Xa, A @ Xa) < 1e-14
    assert last_rows_route(Sa) == (2, 7, 32)
    D = sp.random(200, 300, density=0.5, random_state=rng, data_rvs=rng.standard_normal).tocsr()
    Xd2 = rng.standard_normal((300, 4))
    Sd = pkg.CsrMatrix(D)
    assert rel(Sd @ Xd2, D @ Xd2) < 1e-13
    assert last_rows_route(Sd) == (0, 0, 0)
    # the banded FEM case keeps the plan: a 1-D chain with 3 couplings per row
    T = sp.diags([1.0, -2.5, 1.0], [-1, 0, 1], shape=(5000, 5000)).tocsr()
    Xt = rng.standard_normal((5000, 32))
    assert rel(pkg.CsrMatrix(T) @ Xt, T @ Xt) < 1e-14


def test_darcy_stiffness_assembly_on_device(pkg):
    """SURVEY 8f rank 4, first piece: assemble_darcy_diff_matrix (src/problems/darcy.jl:5-63) on the structured
    P1 mesh, on the device, entry by entry against the oracle (values 1e-14 of max |G|: fixed summation
    order over a node's cells); then the reference's per-problem chain with only the coefficient table
    crossing the bus: table -> G (device) -> Q + Q_eps G'G (device) -> factor -> mean, against the oracle."""
    import torch
    gq = np.linspace(0.0, 1.0, 241)
    GX, GY = np.meshgrid(gq, gq, indexing="ij")
    for n, seed in ((32, 523802340), (64, 11), (256, 7)):
        table = pkg.workloads.darcy_coefficient(seed)(GX.ravel(), GY.ravel()).reshape(241, 241)
        Go, fo = O.assemble_darcy_diff_matrix(n, n, gq, gq, table, 2.0)
        d = pkg.DarcyP1Assembler(n, n)
        vals, f = d.assemble(table, beta=2.0)
        assert np.array_equal(d.pattern.indices, Go.indices)
        assert np.max(np.abs(vals - Go.data)) < 1e-14 * np.max(np.abs(Go.data))
        assert np.max(np.abs(f - fo)) < 1e-14 * np.max(np.abs(fo))      # six cell shares per node, summed in cell order
        vd, fd = d.assemble(torch.from_numpy(table).cuda(), beta=2.0)          # device-resident table and outputs
        assert vd.is_cuda and np.array_equal(vd.cpu().numpy(), vals) and np.array_equal(fd.cpu().numpy(), f)
    # rectangular mesh, another table size
    tab2 = np.random.default_rng(3).uniform(1.0, 5.0, (50, 50))
    g2 = np.linspace(0.0, 1.0, 50)
    Go, fo = O.assemble_darcy_diff_matrix(40, 24, g2, g2, tab2, 1.0)
    v2, f2 = pkg.DarcyP1Assembler(40, 24).assemble(tab2)
    assert np.max(np.abs(v2 - Go.data)) < 1e-14 * np.max(np.abs(Go.data)) and np.max(np.abs(f2 - fo)) < 1e-14 * np.max(np.abs(fo))
    # the problem loop of scripts/darcy/solve_darcy_gmrf-fem.jl:176-190 from the coefficient table on
    n, N, q_eps = 32, 8, 1e8
    Q0, _, _ = pkg.workloads.darcy_conditioning(n)
    d = pkg.DarcyP1Assembler(n, n)
    asm = pkg.PosteriorAssembler(Q0, d.pattern)
    F = None
    qd = torch.from_numpy(Q0.data).cuda()
    w = pkg.workloads.make("darcy32")
    for seed in (523802340, 99):
        table = pkg.workloads.darcy_coefficient(seed)(GX.ravel(), GY.ravel()).reshape(241, 241)
        a_vals, y = d.assemble(torch.from_numpy(table).cuda())
        p_vals = asm.precision(qd, a_vals, q_eps)
        if F is None:
            P = asm.pattern.copy(); P.data = p_vals.cpu().numpy()
            F = pkg.tridiagonal_cholesky(P, N)
        else:
            F.refactor(p_vals)
        rhs = asm.rhs(None, a_vals, torch.zeros(n * n, dtype=torch.float64, device="cuda"), y, q_eps)
        mu = pkg.ldiv(F, rhs)
        Go, fo = O.assemble_darcy_diff_matrix(n, n, gq, gq, table, 1.0)
        _, _, mu_o = O.condition_on_observations(Q0, None, Go, q_eps, fo, N)
        assert mu.is_cuda and rel(mu.cpu().numpy(), mu_o) < solve_tol(w)


def test_persistent_launch_abort_falls_back(pkg):
    """The safety net of the persistent launches (potrf_persist.hpp): every wait is bounded; a wait that gives up raises the abort
    word, every workgroup drains, `factor_finish` sees the word and repeats the numeric phase with the launch-per-step form, which
    the handle then keeps.  Forced here in a child process with GMRF_PERSIST_SPIN_MS=0 (the first wait that has to wait gives up):
    one problem (a launch per block) and a batch of two (a launch per 256-column panel) must report the abort once and return
    bitwise what the other form returns -- and the flag words must be clean for whatever runs next (the last workgroup out
    zeroes them also when the launch was aborted)."""
    import json
    import subprocess
    import sys
    env = dict(_os.environ, GMRF_PERSIST_SPIN_MS="0")
    r = subprocess.run([sys.executable, _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "persist_abort_child.py")],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["single_aborts_after_first"] == 1 and out["single_aborts_after_second"] == 1, out
    assert out["single_aborts_of_the_step_form"] == 0 and out["single_equal"] and out["single_logdet_equal"], out
    assert out["batch_aborts"] == 1 and out["batch_equal"] and out["batch_block_equal"], out
    # round 5: the event is in the statistics (gmrf_stats), the handle's claim on the device's CUs is released, and set_eager
    # cannot re-arm the persistent form of a handle that gave one up
    assert out["single_stats"] == {"persist_aborts": 1, "persist_route": 0, "persist_cus": 0, "persist_refused": 0}, out
    assert out["single_after_set_eager_0"] == {"persist_aborts": 1, "persist_route": 0, "persist_cus": 0, "persist_refused": 0}, out
    # ... and the STEPWISE factorisation (factor_begin / factor_step_async / pack / factor_end: what the shared-factor job runs)
    # looks at the abort word per block range, BEFORE the range is packed: every packed image is the factor's
    assert out["stepwise_aborts"] == 1 and out["stepwise_images_equal"] and out["stepwise_solve_equal"], out


def test_schur_block_assembled_inside_the_coupling_launch(pkg):
    """Round 5, one problem: `S_i = D_i - C C^T` (/root/reference/src/tridiagonal_cholesky.jl:77) used to be "S := -C C^T (GEMM),
    then S += D_i (scatter_block, a launch of its own on the chain of dependent launches)".  Now the workgroups of the coupling
    launch (spmm_bxt_tiles) that zeroed the rows the product does not write zero the whole block and scatter D_i's rows into it,
    and the product accumulates onto it -- the same single rounding fl(D - acc).  set_eager bit 17 keeps the old sequence: the
    factor (L, C, Linv blocks), the log-determinant and a solve must be bitwise equal."""
    for name in ("burgers512x64", "darcy256"):
        w = pkg.workloads.make(name)
        F = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
        G = pkg.TridiagonalCholeskyFactor()
        G.set_eager(Switch.NO_SCATTER_FOLD)
        G.factor(w.Q, w.n_blocks)
        for i in (0, 1, w.n_blocks // 2, w.n_blocks - 1):
            assert np.array_equal(F.chos[i], G.chos[i]), (name, i)
            assert np.array_equal(F.inverses[i], G.inverses[i]), (name, i)
        assert np.array_equal(F.Cs[w.n_blocks - 2], G.Cs[w.n_blocks - 2])
        assert F.logdet() == G.logdet()
        assert np.array_equal(pkg.ldiv(F, w.rhs), pkg.ldiv(G, w.rhs))
        F.refactor(w.Q.data * 1.5)                     # (graph replay: the zeroing is part of every replay)
        G.refactor(w.Q.data * 1.5)
        assert np.array_equal(F.chos[w.n_blocks - 1], G.chos[w.n_blocks - 1])
        del F, G
        import gc; gc.collect()


def F_ref16(F, res, rhs):
    """16 samples with seed 6 by the launch-per-product form (computed once per handle and kept in that handle's `res`:
    a cache keyed by id(F) handed a freed handle's samples to the next handle allocated at the same address)."""
    if "ref16" not in res:
        F.set_eager(Switch.NO_SWEEP_PERSIST)
        res["ref16"] = F.sample(16, mean=res["per_product"][0], seed=6, like=rhs)
        F.set_eager(0)
    return res["ref16"]


def test_persistent_sweeps_of_one_problem_are_the_per_product_sweeps_bitwise(pkg):
    """Round 5: one problem with blocks of 512 .. 1024 runs each sweep (/root/reference/src/tridiagonal_cholesky.jl:24-52) as
    ONE persistent launch (sweep_persist.hpp: the products hand the panel on as a data flow, sentinel-tagged) instead of two
    dependent launches per block (set_eager bit 16 keeps those).  Same decomposition, same summation order: mean, forward-only,
    backward-only solves and samples (k = 16, 64: the MFMA bodies; the k = 1 bodies) are BITWISE those of the launch-per-product
    form, in graph replay and in eager mode; the statistics say which form ran; an in-place solve keeps the launch-per-product
    form (its input would be lost if a persistent launch gave up)."""
    import gc
    import torch
    for name in ("burgers512x64", "darcy256"):
        w = pkg.workloads.make(name)
        rhs = torch.from_numpy(w.rhs).cuda()
        F = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
        st = F.stats()
        assert st["persist_cus"] == 256 and st["persist_refused"] == 0, st        # (the handle holds the whole chip)
        res = {}
        for label, bits in (("persist", 0), ("persist_eager", Switch.EAGER), ("per_product", Switch.NO_SWEEP_PERSIST)):
            F.set_eager(bits)
            mu = pkg.ldiv(F, rhs); s_mu = F.stats()["sweep_persist"]
            yf = pkg.forward_solve(F, rhs)
            xb = pkg.backward_solve(F, rhs)
            X64 = F.sample(64, mean=mu, seed=3, like=rhs); s_x = F.stats()["sweep_persist"]
            X16 = F.sample(16, mean=mu, seed=5, like=rhs)
            res[label] = (mu, yf, xb, X64, X16)
            assert s_mu == s_x == (0 if bits == Switch.NO_SWEEP_PERSIST else 1), (name, label, s_mu, s_x)
        for label in ("persist", "persist_eager"):
            for a, b in zip(res[label], res["per_product"]):
                assert torch.equal(a, b), (name, label)
        F.set_eager(0)
        # consecutive solves with DIFFERENT right-hand sides through the same panels: a value left over from the previous call
        # (in a cache of another XCD, or in a panel the sentinel fill did not cover) would be taken for this call's data
        rhs2 = torch.flip(rhs, dims=[0]) * 0.37 + 1.0
        F.set_eager(Switch.NO_SWEEP_PERSIST); mu2_ref = pkg.ldiv(F, rhs2); xb2_ref = pkg.backward_solve(F, rhs2); F.set_eager(0)
        for it in range(6):
            if it % 2 == 0:
                assert torch.equal(pkg.ldiv(F, rhs), res["per_product"][0]), (name, it)
                assert torch.equal(pkg.backward_solve(F, rhs), res["per_product"][2]), (name, it)
            else:
                assert torch.equal(pkg.ldiv(F, rhs2), mu2_ref), (name, it)
                assert torch.equal(pkg.backward_solve(F, rhs2), xb2_ref), (name, it)
            assert torch.equal(F.sample(16, mean=res["per_product"][0], seed=5 + it % 2, like=rhs),
                               res["per_product"][4] if it % 2 == 0 else F_ref16(F, res, rhs)), (name, it)
        n0 = F.stats()["sweep_persist_launches"]
        buf = rhs.clone()
        torch.cuda.synchronize()                        # (the handle's stream is its own: it does not wait for torch's)
        F._solve(buf, pkg._cabi.SOLVE_FULL, out=buf)                               # in place
        assert F.stats()["sweep_persist"] == 0 and F.stats()["sweep_persist_launches"] == n0
        assert torch.equal(buf, res["per_product"][0])
        assert F.stats()["persist_aborts"] == 0
        r = w.Q @ res["persist"][0].cpu().numpy() - w.rhs
        assert np.linalg.norm(r) / np.linalg.norm(w.rhs) < 1e-8
        # a second one-problem handle beside the first: the chip is taken, it keeps the launch-per-step / per-product forms
        G = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
        sg = G.stats()
        assert sg["persist_cus"] == 0 and sg["persist_refused"] == 1 and sg["persist_route"] == 0, sg
        assert torch.equal(pkg.ldiv(G, rhs), res["per_product"][0]) and G.stats()["sweep_persist"] == 0
        del F, G
        gc.collect()


def test_posterior_in_one_call_is_mean_then_samples_bitwise(pkg):
    """gmrf_bt_posterior: `mean(x_cond)` and `rand(rng, x_cond)` of one factor (scripts/darcy/solve_darcy_gmrf-fem.jl:190-191) in
    ONE call.  Where the handle's sweeps are persistent launches the samples' backward sweep runs BESIDE the mean's two sweeps
    (a second stream, panels of its own); the results are bitwise those of `ldiv` followed by `sample(mean = ...)` -- with the
    persistent sweeps, with a launch per product, on device tensors and on host arrays (the call is then the two calls), for
    one configuration with persistent sweeps (burgers512x64, darcy256) and one without (darcy64: blocks of 256)."""
    import gc
    import torch
    for name in ("burgers512x64", "darcy256", "darcy64"):
        w = pkg.workloads.make(name)
        rhs = torch.from_numpy(w.rhs).cuda()
        F = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
        mu_ref = pkg.ldiv(F, rhs)
        for k, seed in ((64, 3), (16, 5), (48, 7)):
            X_ref = F.sample(k, mean=mu_ref, seed=seed, like=rhs)
            for bits in (0, Switch.NO_SWEEP_PERSIST, Switch.EAGER):
                F.set_eager(bits)
                mu, X = F.posterior(rhs, k, seed=seed)
                assert torch.equal(mu, mu_ref) and torch.equal(X, X_ref), (name, k, bits)
                st = F.stats()
                assert st["persist_aborts"] == 0
                assert st["sweep_persist"] == (1 if bits != Switch.NO_SWEEP_PERSIST and name != "darcy64" else 0), (name, bits, st["sweep_persist"])
            F.set_eager(0)
        # twice in a row with another right-hand side (the panels of the two streams are reused), then host arrays
        rhs2 = torch.flip(rhs, dims=[0]) * 0.5 - 2.0
        mu2_ref = pkg.ldiv(F, rhs2); X2_ref = F.sample(32, mean=mu2_ref, seed=11, like=rhs)
        for it in range(3):
            mu2, X2 = F.posterior(rhs2, 32, seed=11)
            assert torch.equal(mu2, mu2_ref) and torch.equal(X2, X2_ref), (name, it)
        mu_h, X_h = F.posterior(w.rhs, 16, seed=5)
        assert np.array_equal(mu_h, mu_ref.cpu().numpy()) and np.array_equal(X_h, F.sample(16, mean=mu_ref, seed=5, like=rhs).cpu().numpy())
        del F
        gc.collect()


def test_persistent_sweeps_under_uneven_load(pkg):
    """The hand-offs of the persistent sweeps (data-tagged: a consumer repeats its `sc1` loads of a panel chunk until no value
    is the sentinel) must hold when the chip is NOT idle -- the guide's rule for every inter-workgroup hand-off: test under
    uneven load, checking every word.  A second host thread keeps a batch of 16 darcy256-sized problems (blocks of 1024: GEMMs
    and `potrf_persist`-free batch routes on another stream) factoring and solving while the one-problem handle runs 30
    solves and samples as persistent launches: every result bitwise the launch-per-product result taken on the idle chip;
    no abort."""
    import threading
    import torch
    w = pkg.workloads.make("burgers512x64")
    rhs = torch.from_numpy(w.rhs).cuda()
    F = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
    F.set_eager(Switch.NO_SWEEP_PERSIST)
    mu0 = pkg.ldiv(F, rhs); X0 = F.sample(16, mean=mu0, seed=9, like=rhs)
    F.set_eager(0)
    streams = pkg.StreamSet(1)
    stop = threading.Event()
    err = []
    def load():
        try:
            B = 16
            Fb = pkg.TridiagonalCholeskyFactor(batch=B, stream=streams.pointers[0])
            vals = np.stack([w.Q.data * (1.0 + 0.01 * p) for p in range(B)])
            Fb.factor(w.Q, w.n_blocks, values=vals)
            rb = np.stack([w.rhs] * B)[:, None, :]
            while not stop.is_set():
                Fb.refactor(vals)
                Fb.solve_batch(rb)
            Fb.close()
        except Exception as e:      # noqa: BLE001
            err.append(repr(e))
    th = threading.Thread(target=load)
    th.start()
    try:
        bad = 0
        for it in range(30):
            if it % 3 == 2:
                mu, X = F.posterior(rhs, 16, seed=9)       # (the samples' sweep beside the mean's two: three persistent launches in flight)
            else:
                mu = pkg.ldiv(F, rhs)
                X = F.sample(16, mean=mu, seed=9, like=rhs)
            bad += int(not torch.equal(mu, mu0)) + int(not torch.equal(X, X0))
        st = F.stats()
    finally:
        stop.set(); th.join()
    assert not err, err
    assert bad == 0 and st["persist_aborts"] == 0 and st["sweep_persist"] == 1, (bad, st["persist_aborts"], st["sweep_persist"])
    del F
    import gc; gc.collect()


def test_persistent_sweep_abort_falls_back(pkg):
    """The safety net of the persistent sweeps: every wait for an input panel is bounded; a wave that gives up raises the abort
    words, every other wait ends on them, the launch drains; gmrf_bt_solve / gmrf_bt_sample / gmrf_bt_posterior and the sampled
    variances see the (mapped host) word behind their own synchronisation and repeat the call with a launch per product, which the
    handle keeps (stats.persist_aborts, claim released); aliased calls keep that form from the start.  Forced in a child process
    with GMRF_SWEEP_SPIN_MS=0: results bitwise those of the launch-per-product form."""
    import json
    import subprocess
    import sys
    env = dict(_os.environ, GMRF_SWEEP_SPIN_MS="0")
    r = subprocess.run([sys.executable, _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "sweep_abort_child.py")],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["after_factor"] == {"persist_aborts": 0, "persist_cus": 256, "sweep_persist": 0}, out
    assert out["after_solve"] == {"persist_aborts": 1, "persist_cus": 0, "sweep_persist": 0}, out
    assert out["after_sample"] == {"persist_aborts": 1, "persist_cus": 0, "sweep_persist": 0}, out
    assert out["route_after_refactor"] == 0 and out["aborts_of_the_per_product_form"] == 0, out
    assert out["solve_equal"] and out["sample_equal"], out
    assert out["sample_first"] == {"persist_aborts": 1, "persist_cus": 0, "sweep_persist": 0} and out["sample_first_equal"], out
    # the sampled variances (gmrf_bt_marginal_var, gmrf_bt_var_accumulate, gmrf_bt_marginal_var_batch on a batch of one) and two
    # aliased calls, each the first persistent sweep of a fresh handle: bitwise the per-product handle's results; where a persistent
    # launch ran it gave up once and the handle let go of the chip (the aliased sample keeps the per-product form from the start)
    for name in ("var_mc_65", "var_rbmc_50", "var_accumulate_mc_dev", "var_accumulate_rbmc_host", "var_batch_rbmc_65",
                 "sample_mean_is_out", "posterior_b_in_samples"):
        r = out[name]
        assert r["equal"] and r["persist_cus_before"] == 256 and r["persist_aborts"] <= 1, (name, r)
        assert r["launches"] == 0 or (r["persist_aborts"] == 1 and r["persist_cus"] == 0), (name, r)
        if not name.startswith("sample"):
            assert r["launches"] > 0, (name, r)


# ---- the persistent sweeps (one problem, blocks of 512 .. 1024) against a float64 reference, and with aliased arguments
_PERSIST_REF = {}


def _persist_case(pkg, name):
    """(w, Fo, tol, F): the oracle factor (kept per workload: plain NumPy) and a FRESH one-problem handle that holds the whole chip,
    so that its sweeps are persistent launches (the caller closes it: the next fresh handle needs the chip)."""
    if name not in _PERSIST_REF:
        w = pkg.workloads.make(name)
        if name == "darcy256":
            w.meta.setdefault("cond", 3.4e9)       # (as in test_config_darcy256_against_oracle: eigsh at n = 65536 takes minutes)
        _PERSIST_REF[name] = (w, O.tridiagonal_cholesky(w.Q, w.n_blocks), solve_tol(w))
    w, Fo, tol = _PERSIST_REF[name]
    F = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
    st = F.stats()
    assert st["persist_cus"] == 256 and st["persist_refused"] == 0, (name, st)
    return w, Fo, tol, F


def _release(F):
    import gc
    F.close()
    gc.collect()


@pytest.mark.parametrize("name", ["burgers512x64", "darcy256"])
def test_persistent_sampled_variances_against_float64_reference(pkg, name):
    """RBMCStrategy(k) and plain MC variances (`std(x_cond)`, scripts/darcy/solve_darcy_gmrf-fem.jl:192) where the samples' sweeps
    are persistent launches: against the float64 oracle on the same Philox draws, for k = 1 (the k = 1 body), 17 (a padded 32-wide
    panel), 50 (the padded 64-wide panel of RBMCStrategy(50)), 64, 65 (64 + a k = 1 tail chunk) and 130 (three chunks); bitwise the
    launch-per-product form; the statistics say which form ran and count one launch per chunk of 64.  Then into a device tensor, and
    sharded over two calls of var_accumulate (host and device accumulators) against the one-shot estimator."""
    import torch
    w, Fo, tol, F = _persist_case(pkg, name)
    try:
        Q = pkg.CsrMatrix(w.Q)
        seed = 41
        X130 = O.backward_solve(Fo, F.normals(130, seed=seed))      # (Philox draws: the first k columns are the draws of k samples)
        # MC at k = 1 is x^2, arbitrarily close to zero at some node: its error is taken against the node's variance (130 samples)
        scale = O.marginal_variances_mc(X130)
        one_shot = {}
        for k in (1, 17, 50, 64, 65, 130):
            X = X130[:, :k]
            for method in ("rbmc", "mc"):
                kw = dict(k=k, seed=seed, Q=Q) if method == "rbmc" else dict(k=k, seed=seed)
                ref = O.marginal_variances_rbmc(w.Q, X) if method == "rbmc" else O.marginal_variances_mc(X)
                n0 = F.stats()["sweep_persist_launches"]
                v = F.marginal_var(method, **kw)
                st = F.stats()
                assert st["sweep_persist"] == 1 and st["sweep_persist_launches"] - n0 == -(-k // 64), (name, method, k, st)
                den = ref if method == "rbmc" else np.maximum(ref, scale)
                err = float(np.max(np.abs(v - ref) / den))
                assert err < 4.0 * tol, (name, method, k, err, tol)             # squares of samples that agree to tol
                F.set_eager(Switch.NO_SWEEP_PERSIST)
                v_pp = F.marginal_var(method, **kw)
                st_pp = F.stats()
                F.set_eager(0)
                assert st_pp["sweep_persist"] == 0 and st_pp["sweep_persist_launches"] == st["sweep_persist_launches"], (name, method, k)
                assert np.array_equal(v, v_pp), (name, method, k)
                one_shot[(method, k)] = v
        out = torch.full((w.n,), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()                        # (the handle's stream is its own: it does not wait for torch's)
        F.marginal_var("rbmc", k=50, seed=seed, Q=Q, out=out)
        assert F.stats()["sweep_persist"] == 1
        assert np.array_equal(out.cpu().numpy(), one_shot[("rbmc", 50)]), name
        # sharded: samples [0, 70) then [70, 130) into one accumulator
        inv_d = 1.0 / sp.csr_matrix(w.Q).diagonal()
        for method in ("mc", "rbmc"):
            for on_dev in (False, True):
                acc = torch.zeros(w.n, dtype=torch.float64, device="cuda") if on_dev else np.zeros(w.n)
                torch.cuda.synchronize()                # (the handle's stream is its own: it does not wait for torch's)
                F.var_accumulate(acc, method, 0, 70, seed=seed, Q=Q if method == "rbmc" else None)
                assert F.stats()["sweep_persist"] == 1
                F.var_accumulate(acc, method, 70, 60, seed=seed, Q=Q if method == "rbmc" else None)
                a = acc.cpu().numpy() if on_dev else acc
                v = a / 130.0 + (inv_d if method == "rbmc" else 0.0)
                ref = one_shot[(method, 130)]
                assert float(np.max(np.abs(v - ref) / ref)) < 1e-12, (name, method, on_dev)
        assert F.stats()["persist_aborts"] == 0
    finally:
        _release(F)


@pytest.mark.parametrize("name", ["burgers512x64", "darcy256"])
def test_persistent_sweeps_c_abi_leading_dimensions_and_mixed_k(pkg, lib, name):
    """Straight through the C ABI on the persistent sweeps: n x k right-hand sides with ld = n + 7 (host and device memory), the
    three solve modes and samples with a given z, k changing from call to call on one handle (1, 2, 16, 17, 64, 128, 129: the
    k = 1 body, padded panels, one chunk of 128, 128 + 1).  Against the oracle; bitwise the same calls with a launch per product;
    the NaN padding of the leading dimension is neither read into the result nor written."""
    import torch
    w, Fo, tol, F = _persist_case(pkg, name)
    cabi = pkg._cabi
    try:
        n, ld = w.n, w.n + 7
        rng = np.random.default_rng(5)
        mu = O.ldiv(Fo, w.rhs)
        mu_dev = torch.from_numpy(mu).cuda()
        oracle = {cabi.SOLVE_FULL: O.ldiv, cabi.SOLVE_FORWARD: O.forward_solve, cabi.SOLVE_BACKWARD: O.backward_solve}

        def padded(M, dev):
            buf = np.full((M.shape[1], ld), np.nan)
            buf[:, :n] = M.T
            return torch.from_numpy(buf).cuda() if dev else buf

        def fetch(buf):
            return buf.cpu().numpy() if isinstance(buf, torch.Tensor) else buf

        def both_forms(call, dev, k):
            """call(out) on the persistent form and on the launch-per-product form; the first result (host array)"""
            res = []
            for bits in (0, Switch.NO_SWEEP_PERSIST):
                F.set_eager(bits)
                out = padded(np.full((n, k), np.nan), dev)
                n0 = F.stats()["sweep_persist_launches"]
                cabi.check(call(out))
                st = F.stats()
                assert st["sweep_persist"] == (1 if bits == 0 else 0), (name, k, bits, st["sweep_persist"])
                assert (st["sweep_persist_launches"] > n0) == (bits == 0), (name, k, bits)
                res.append(fetch(out))
            F.set_eager(0)
            a, b = res
            assert np.array_equal(a[:, :n], b[:, :n]), (name, k, dev)
            assert np.all(np.isnan(a[:, n:])) and np.all(np.isnan(b[:, n:])), (name, k, dev)
            return a[:, :n].T

        for k in (1, 2, 16, 17, 64, 128, 129, 1):
            B = rng.standard_normal((n, k))
            for dev in (False, True):
                b = padded(B, dev)
                b0 = fetch(b).copy()
                for mode in (cabi.SOLVE_FULL, cabi.SOLVE_FORWARD, cabi.SOLVE_BACKWARD):
                    y = both_forms(lambda out: lib.gmrf_bt_solve(F._h, cabi.ptr(b), cabi.ptr(out), k, ld, ld, mode), dev, k)
                    assert rel(y, oracle[mode](Fo, B)) < tol, (name, k, dev, mode)
                # samples mean + L^-T z with the caller's z (ld > n) and the oracle's mean
                m = mu_dev if dev else mu
                x = both_forms(lambda out: lib.gmrf_bt_sample(F._h, 0, 0, k, cabi.ptr(m), cabi.ptr(b), cabi.ptr(out), ld), dev, k)
                assert rel(x, O.sample(Fo, mu, B)) < tol, (name, k, dev)
                assert np.array_equal(fetch(b), b0, equal_nan=True), (name, k, dev)       # the inputs are not written
        assert F.stats()["persist_aborts"] == 0
    finally:
        _release(F)


@pytest.mark.parametrize("name", ["burgers512x64", "darcy256"])
def test_persistent_sweeps_with_aliased_arguments(pkg, lib, name):
    """Arguments that overlap (well defined with a launch per product for k <= 128: every input is packed whole into the panels
    before any output is written): a sample whose mean IS its output (k = 1), a sample whose z lies one column before its output,
    a solve whose y lies one column after b, a posterior whose b is column 0 of its samples.  Each is bitwise the same aliased call
    with a launch per product (these calls keep that form: a persistent launch that gave up could not be repeated from inputs it
    has overwritten); the samples agree with the oracle."""
    import torch
    w, Fo, tol, F = _persist_case(pkg, name)
    cabi = pkg._cabi
    try:
        n, ld, k, seed = w.n, w.n + 5, 16, 23
        mu_o = O.ldiv(Fo, w.rhs)
        rhs = torch.from_numpy(w.rhs).cuda()
        mu = pkg.ldiv(F, rhs).cpu().numpy()
        z1 = F.normals(1, seed=seed)
        Z = np.random.default_rng(8).standard_normal((n, k))

        def fetch(buf):
            return buf.cpu().numpy() if isinstance(buf, torch.Tensor) else buf.copy()

        def both_forms(run):
            res = [None, None]
            for i, bits in enumerate((0, Switch.NO_SWEEP_PERSIST)):
                F.set_eager(bits)
                res[i] = run()
            F.set_eager(0)
            return res

        for dev in (False, True):
            wrap = (lambda a: torch.from_numpy(a).cuda()) if dev else (lambda a: a)

            def mean_is_out():
                buf = wrap(mu.copy())
                cabi.check(lib.gmrf_bt_sample(F._h, seed, 0, 1, cabi.ptr(buf), None, cabi.ptr(buf), n))
                return fetch(buf)
            a, b = both_forms(mean_is_out)
            assert np.array_equal(a, b), (name, dev)
            assert rel(a, mu_o + O.backward_solve(Fo, z1)[:, 0]) < tol, (name, dev)

            def z_before_out():
                buf = np.full((k + 1, ld), np.nan)
                buf[:k, :n] = Z.T
                buf = wrap(buf)
                base = buf.data_ptr() if dev else buf.ctypes.data
                mean = wrap(mu.copy())
                cabi.check(lib.gmrf_bt_sample(F._h, 0, 0, k, cabi.ptr(mean), cabi.ptr(base), cabi.ptr(base + 8 * ld), ld))
                return fetch(buf)
            a, b = both_forms(z_before_out)
            assert np.array_equal(a, b, equal_nan=True), (name, dev)
            assert np.all(np.isnan(a[:, n:])), (name, dev)
            assert rel(a[1:, :n].T, O.sample(Fo, mu_o, Z)) < tol, (name, dev)

            def y_after_b():
                buf = np.full((k + 1, ld), np.nan)
                buf[:k, :n] = Z.T
                buf = wrap(buf)
                base = buf.data_ptr() if dev else buf.ctypes.data
                cabi.check(lib.gmrf_bt_solve(F._h, cabi.ptr(base), cabi.ptr(base + 8 * ld), k, ld, ld, cabi.SOLVE_FULL))
                return fetch(buf)
            a, b = both_forms(y_after_b)
            assert np.array_equal(a, b, equal_nan=True), (name, dev)
            assert rel(a[1:, :n].T, O.ldiv(Fo, Z)) < tol, (name, dev)

        # posterior, b = column 0 of the samples (device memory: where the samples' sweep may run beside the mean's)
        mu_ref = pkg.ldiv(F, rhs)
        X_ref = F.sample(k, mean=mu_ref, seed=seed, like=rhs)

        def b_in_samples():
            samples = torch.full((k, n), float("nan"), dtype=torch.float64, device="cuda")
            samples[0] = rhs
            torch.cuda.synchronize()                    # (the handle's stream is its own: it does not wait for torch's)
            mean = torch.empty(n, dtype=torch.float64, device="cuda")
            cabi.check(lib.gmrf_bt_posterior(F._h, cabi.ptr(samples[0]), seed, 0, k, cabi.ptr(mean), cabi.ptr(samples), n))
            return mean, samples
        (ma, sa), (mb, sb) = both_forms(b_in_samples)
        assert torch.equal(ma, mb) and torch.equal(sa, sb), name
        assert torch.equal(ma, mu_ref) and torch.equal(sa, X_ref.t()), name
        assert F.stats()["persist_aborts"] == 0
    finally:
        _release(F)


@pytest.mark.parametrize("name", ["burgers512x64", "darcy256"])
def test_persistent_route_does_not_depend_on_the_previous_call(pkg, name):
    """An in-place solve keeps the launch-per-product form for ITSELF only: the variances and the one-call posterior that follow
    run their sweeps as persistent launches again (sweep_persist says so), with results bitwise those of the per-product form; the
    posterior runs the samples' sweep beside the mean's (its sample_ms is 0: the call is not solve + sample)."""
    import torch
    w, Fo, tol, F = _persist_case(pkg, name)
    try:
        rhs = torch.from_numpy(w.rhs).cuda()
        F.set_eager(Switch.NO_SWEEP_PERSIST)
        mu_ref = pkg.ldiv(F, rhs)
        X_ref = F.sample(16, mean=mu_ref, seed=7, like=rhs)
        v_ref = F.marginal_var("mc", k=64, seed=5)
        F.set_eager(0)
        buf = rhs.clone()
        torch.cuda.synchronize()                        # (the handle's stream is its own: it does not wait for torch's)
        F._solve(buf, pkg._cabi.SOLVE_FULL, out=buf)                               # in place
        assert F.stats()["sweep_persist"] == 0 and torch.equal(buf, mu_ref)
        v = F.marginal_var("mc", k=64, seed=5)
        assert F.stats()["sweep_persist"] == 1, name
        assert np.array_equal(v, v_ref), name
        buf = rhs.clone()
        torch.cuda.synchronize()                        # (the handle's stream is its own: it does not wait for torch's)
        F._solve(buf, pkg._cabi.SOLVE_FULL, out=buf)
        assert F.stats()["sweep_persist"] == 0
        mu, X = F.posterior(rhs, 16, seed=7)
        st = F.stats()
        assert st["sweep_persist"] == 1 and st["sample_ms"] == 0.0, (name, st["sweep_persist"], st["sample_ms"])
        assert torch.equal(mu, mu_ref) and torch.equal(X, X_ref), name
        assert st["persist_aborts"] == 0
    finally:
        _release(F)


def test_inverse_rows_inside_the_fused_steps(pkg):
    """One problem, blocks of up to 16 tiles: the inverse Linv_i is assembled row by row by extra workgroups of
    the fused panel-step launches (block forward substitution, X[r,c] = -X_rr sum_p L[r,p] X[p,c]) instead of by
    recursive doubling after them (set_eager bit 7 keeps the doubling).  Same L bitwise; Linv, C and the
    solves to rounding; both against the oracle; L Linv = I to the conditioning of the block."""
    for name in ("darcy64", "burgers512x64", "darcy256"):
        w = pkg.workloads.make(name)
        if name == "darcy256":
            w.meta.setdefault("cond", 3.4e9)
        Fr = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
        Fd = pkg.TridiagonalCholeskyFactor()
        Fd.set_eager(Switch.DOUBLING_INVERSE)
        Fd.factor(w.Q, w.n_blocks)
        i = w.n_blocks // 2
        assert np.array_equal(Fr.chos[0], Fd.chos[0])
        Xr, Xd = Fr.get_block(pkg._cabi.BLOCK_LINV, i), Fd.get_block(pkg._cabi.BLOCK_LINV, i)
        L = np.tril(Fr.chos[i])
        scale = np.max(np.abs(Xd))
        assert np.max(np.abs(Xr - Xd)) / scale < 1e-10
        eye = np.eye(L.shape[0])
        err_r, err_d = np.max(np.abs(L @ Xr - eye)), np.max(np.abs(L @ Xd - eye))
        assert err_r <= 4.0 * err_d + 1e-13, (err_r, err_d)          # substitution is at least as accurate as doubling
        assert np.allclose(np.triu(Xr, 1), 0.0)
        tol = solve_tol(w)
        x_r, x_d = pkg.ldiv(Fr, w.rhs), pkg.ldiv(Fd, w.rhs)
        assert rel(x_r, x_d) < tol
        if name != "darcy256":
            assert rel(x_r, O.ldiv(O.tridiagonal_cholesky(w.Q, w.n_blocks), w.rhs)) < tol
        qn = abs(w.Q).sum(axis=1).max()
        assert np.linalg.norm(w.Q @ x_r - w.rhs) / (qn * np.linalg.norm(x_r) + np.linalg.norm(w.rhs)) < 1e-14
        # the look-ahead chain (tile j+1 factored inside the launch of step j) does the same arithmetic as the form in
        # which every workgroup of a step re-factors the diagonal tile (set_eager bit 8): bitwise equal factor
        Fn = pkg.TridiagonalCholeskyFactor()
        Fn.set_eager(Switch.NO_LOOKAHEAD)
        Fn.factor(w.Q, w.n_blocks)
        for b in (0, i, w.n_blocks - 1):
            assert np.array_equal(Fr.chos[b], Fn.chos[b])
            assert np.array_equal(Fr.get_block(pkg._cabi.BLOCK_LINV, b), Fn.get_block(pkg._cabi.BLOCK_LINV, b))
        assert np.array_equal(x_r, pkg.ldiv(Fn, w.rhs))
    # a non-SPD block is still reported with its index by the look-ahead chain
    w = pkg.workloads.make("darcy64")
    Qc = w.Q.tocsc()
    bad = Qc.data.copy()
    d = np.flatnonzero((Qc.indices == 1000) & (np.repeat(np.arange(w.n), np.diff(Qc.indptr)) == 1000))[0]
    bad[d] = -1e20
    F = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
    with pytest.raises(pkg.NotPositiveDefinite) as e:
        F.refactor(bad)
    assert e.value.info == 1000 // w.block_size + 1


def test_burgers_tangent_on_device_and_resident_gauss_newton(pkg):
    """SURVEY 8f rank 4, second piece: f_and_J of scripts/burgers/solve_burgers_gmrf-fem.jl:118-149 (advection tangent
    src/problems/burgers.jl:5-59 per time slice + the static mass / diffusion part) on the device, entry by entry
    against the oracle (1e-14 of max |J|: two cells per row, fixed order); then Gauss-Newton iterations
    (scripts/solve_burger.jl:143-149) in which NOTHING crosses the bus: w -> (J values, f) -> Q + noise J'J and the
    right-hand side -> re-factor -> solve, all on device tensors, against the oracle's iteration."""
    import torch
    rng = np.random.default_rng(8)
    for ns, nt in ((16, 5), (512, 64), (4096, 6)):
        dt, nu = 1.0 / (nt - 1), 0.01 / np.pi
        w = rng.standard_normal(ns * nt)
        fo, Jo = O.burgers_f_and_J(ns, nt, dt, nu, w)
        b = pkg.BurgersP1Tangent(ns, nt, dt, nu)
        vals, f = b.tangent(w)
        assert np.array_equal(b.pattern.indices, Jo.indices)
        assert np.max(np.abs(vals - Jo.data)) < 1e-14 * np.max(np.abs(Jo.data))
        assert np.max(np.abs(f - fo)) < 1e-13 * max(np.max(np.abs(fo)), 1.0)
        vd, fd = b.tangent(torch.from_numpy(w).cuda())
        assert vd.is_cuda and np.array_equal(vd.cpu().numpy(), vals) and np.array_equal(fd.cpu().numpy(), f)
    # device-resident Gauss-Newton on the Burgers prior of the packaged workload (prior + initial condition in Q)
    ns, nt = 64, 8
    gn = pkg.workloads.burgers_gauss_newton(ns, nt)
    dt, nu, noise, N = 1.0 / (nt - 1), 0.01 / np.pi, gn["noise"], gn["n_blocks"]
    b = pkg.BurgersP1Tangent(ns, nt, dt, nu)
    asm = pkg.PosteriorAssembler(gn["Q"], b.pattern)
    qd = torch.from_numpy(gn["Q"].data).cuda(); qx = torch.from_numpy(gn["Qx_prior"]).cuda()
    x_dev = torch.from_numpy(gn["x_prior"].copy()).cuda()
    xs = np.arange(ns) / ns
    x_dev[:ns] = torch.from_numpy(np.sin(2 * np.pi * xs)).cuda()          # a non-trivial starting point
    xo = x_dev.cpu().numpy().copy()
    F = None
    for it in range(3):
        jv, fv = b.tangent(x_dev)                                           # device in, device out
        if F is None:
            P = asm.pattern.copy(); P.data = asm.precision(qd, jv, noise).cpu().numpy()
            F = pkg.tridiagonal_cholesky(P, N)
        x_dev = pkg.gn_step(F, asm, qd, qx, jv, x_dev, -fv, noise)
        fo, Jo = O.burgers_f_and_J(ns, nt, dt, nu, xo)
        xo = O.gn_step(gn["Q"], Jo, gn["Qx_prior"], xo, -fo, noise, N)
        assert x_dev.is_cuda and rel(x_dev.cpu().numpy(), xo) < 1e-9


def test_spmm_stream_ordered_variants(pkg):
    """gmrf_spmm_async / gmrf_spmm_rows_async: device operands, enqueued on the matrix's stream without a host
    synchronisation; results bitwise those of the synchronous calls; host pointers are refused."""
    import torch
    w = pkg.workloads.make("darcy64")
    st = torch.cuda.current_stream()
    S = pkg.CsrMatrix(w.Q, stream=st.cuda_stream)
    x = torch.randn(w.n, dtype=torch.float64, device="cuda")
    X = torch.randn(w.n, 16, dtype=torch.float64, device="cuda")
    y, Y = torch.empty_like(x), torch.empty_like(X)
    for _ in range(3):                                  # back to back, no synchronisation in between
        S.matmul_into(x, y); S.matmul_into(X, Y)
    torch.cuda.synchronize()
    assert torch.equal(y, S @ x) and torch.equal(Y, S @ X)
    assert np.max(np.abs(y.cpu().numpy() - w.Q @ x.cpu().numpy())) < 1e-12 * np.max(np.abs(y.cpu().numpy()))
    with pytest.raises(TypeError):
        S.matmul_into(x.cpu(), y)
    lib = pkg._cabi.load()
    xh = np.zeros(w.n)
    assert lib.gmrf_spmm_async(S._h, pkg._cabi.ptr(xh), pkg._cabi.ptr(y), 1, w.n, w.n) == pkg._cabi.ERR_BAD_SHAPE


# ----------------------------------------------------------------------------- round 3: the path bench.py times

def _darcy_batch(pkg, n_xy, B, n_distinct=8):
    """B problems on one mesh as bench.py's ProblemsJob builds them: n_distinct coefficient fields (seeds
    523802340 + p), problem p of the batch takes field p % n_distinct."""
    w = pkg.workloads.darcy(n_xy)
    vals, rhs = [w.Q.data], [w.rhs]
    for p in range(1, min(B, n_distinct)):
        wp = pkg.workloads.darcy(n_xy, seed=523802340 + p)
        assert wp.Q.nnz == w.Q.nnz and np.array_equal(wp.Q.indices, w.Q.indices)
        vals.append(wp.Q.data); rhs.append(wp.rhs)
    idx = [p % len(vals) for p in range(B)]
    return w, np.stack([vals[i] for i in idx]), np.stack([rhs[i] for i in idx])


def test_measured_path_darcy256_batch_against_oracle(pkg):
    """The code path the headline number is measured on -- darcy256, a batch of 64 problems (bench.py's default; 8 distinct coefficient
    fields, as bench.py cycles them: every launch has the grid and the kernel symbol of the timed job),
    keep_l = 0, on a StreamSet stream, HipEngine / ShardedPosterior.step with the second step replayed from the
    captured graphs (128-column diagonal blocks + GEMM panels + rank-256 GEMM updates on the LDS-DMA kernel, doubling
    assembly of Linv, spmm_bxt_tiles, GEMM-route k = 64 sweeps, Philox sample_batch) -- against the oracle at FULL size for two
    problems of the batch: mean, the 64 samples (device draws fetched with gmrf_bt_normals), logdet, exact and
    RBMC(50) variances of the last eight blocks.  Tolerances as in test_config_darcy256_against_oracle; the
    variance tolerance is backed here by an extended-precision reference (HIP error <= 2 x the oracle's)."""
    from importlib import import_module
    from tests import measured_path as MP
    post = import_module(pkg.__name__ + ".posterior")
    w, vals, rhs = _darcy_batch(pkg, 256, 64)
    w.meta.setdefault("cond", 3.4e9)
    tol = solve_tol(w)
    res = MP.run(pkg, post, O, w.Q, w.n_blocks, vals, rhs, k_samples=64, check=(1, 62), last_blocks=8, rbmc_k=50,
                 true_var_samples=24)
    print("measured path:", res)
    route = res["route"]
    # the launch classes of the timed route (include/gmrf_hip.h, gmrf_stats): both symbols of the LDS-DMA GEMM, the
    # 128-column diagonal-block kernel, the sparse coupling product, k = 1 sweeps; none of the one-problem kernels
    # (fused potrf_step, sweep_mm) and none of the round-2 rank-64 step kernels
    for cls in (14, 15, 16, 10, 3):
        assert route.get(cls, 0) > 0, (cls, route)
    for cls in (1, 2, 8, 9):
        assert route.get(cls, 0) == 0, (cls, route)
    for p in (1, 62):
        r = res[p]
        assert r["mean_rel_l2"] < tol and r["samples_rel_l2"] < tol, r
        assert r["logdet_rel"] < 1e-10, r
        assert r["var_rbmc_max_rel"] < 4.0 * tol, r               # squares of samples that agree to tol
        assert r["var_rbmc_vs_exact_median_rel"] < 0.25, r        # RBMCStrategy(50) estimates the same variances (median error 0.11-0.14)
        # exact variances: both selected inversions sit at O(cond * eps) from the truth; the HIP one is no further
        # from it than twice the LAPACK-backed oracle, so the two cannot be asked to agree better than ~3 x that
        assert r["var_err_hip_vs_true"] <= 2.0 * r["var_err_oracle_vs_true"] + 1e-13, r
        assert r["var_exact_max_rel"] < max(1e-9, 0.01 * w.meta["cond"] * EPS), r


def test_measured_path_elliptic512_batch8_against_oracle(pkg):
    """BASELINE config C4 on the route its bench line is TIMED on: elliptic512 (512 x 512 nodes, blocks of
    1024; the leading 128 of its 256 blocks) as a batch of 8 problems -- the pattern's values scaled per problem, as bench.py's ProblemsJob builds a non-Darcy batch --
    keep_l = 0, on a StreamSet stream, HipEngine / ShardedPosterior.step replayed from its graphs: every 256-column panel's
    diagonal block is ONE persistent launch on 7 workgroups per problem (potrf_persist, kernel class 17; no potrf_diag128), the
    rest 32 x 32- and 64 x 64-tile GEMMs.  One problem of the batch against the oracle at FULL block size: mean, 32 samples
    (device draws fetched with gmrf_bt_normals), log-determinant, exact and RBMC variances of the last two blocks."""
    from importlib import import_module
    from tests import measured_path as MP
    post = import_module(pkg.__name__ + ".posterior")
    w = pkg.workloads.make("elliptic512")
    w.meta.setdefault("cond", 4.04e9)          # (lmax * ||Q^-1|| by eigsh / SuperLU: 90 s of host time, measured once)
    B = 8
    # the leading 128 of the 256 blocks: same block size, batch, launches per block and kernels as the timed job, half the chain
    # (the oracle's dense blocks of the whole chain alone take ~3 minutes of host time)
    nbk = 128
    ns = nbk * w.block_size
    Qs = w.Q.tocsr()[:ns, :ns].tocsc(); Qs.sort_indices()
    vals = np.stack([Qs.data * (1.0 + 0.01 * p) for p in range(B)])
    rhs = np.stack([w.rhs[:ns]] * B)
    tol = solve_tol(w)
    res = MP.run(pkg, post, O, Qs, nbk, vals, rhs, k_samples=32, check=(5,), last_blocks=2, rbmc_k=16)
    print("measured path (elliptic512, batch 8):", res, "cond", w.meta["cond"])
    route = res["route"]
    assert route.get(17, 0) == (w.block_size // 256) * nbk, route                 # one persistent launch per panel
    for cls in (16, 1, 8, 9):
        assert route.get(cls, 0) == 0, (cls, route)
    assert route.get(14, 0) + route.get(15, 0) + route.get(13, 0) > 0, route
    r = res[5]
    assert r["mean_rel_l2"] < tol and r["samples_rel_l2"] < tol, (r, tol)
    assert r["logdet_rel"] < 1e-10, r
    assert r["var_exact_max_rel"] < max(1e-9, 0.01 * w.meta["cond"] * EPS), r
    assert r["var_rbmc_max_rel"] < 4.0 * tol, r


def test_bench_plain_line_and_full_legs(tmp_path):
    """bench.py as a child on a small job (darcy64, one stream x batch 8): a plain run is the headline alone -- its line says
    what the timed steps did (value x ms_per_step = the solves of one step), --dump-outputs writes the last step's means and
    samples, and none of the legs --full adds has run; --full adds them after the timed steps (here the instrumented step,
    its roofline and the phase times: the costlier legs are left out by their --no-* options)."""
    import json
    import subprocess
    import sys
    bench = _os.path.join(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))), "bench.py")
    job = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--config", "darcy64", "--streams", "1", "--batch", "8"]
    added = ("roofline", "kernels", "phases_ms", "gemm_by_shape", "single_problem", "full_loop", "roofline_spmm", "cpu_baseline", "parity")

    def run(*extra):
        r = subprocess.run([sys.executable, bench] + job + list(extra), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return json.loads(r.stdout.strip().splitlines()[-1])

    plain = run("--dump-outputs", str(tmp_path))
    assert plain["unit"] == "solves/s" and plain["higher_is_better"] is True and plain["dtype"] == "f64"
    assert plain["steps"] == 2 and plain["warmup"] == 1 and plain["value"] > 0
    assert abs(plain["value"] * plain["ms_per_step"] * 1e-3 - 8 * 65) < 1e-6 * 8 * 65
    assert plain["persist_aborts"] == 0
    assert not [k for k in added if k in plain], sorted(plain)
    mean, samples = np.load(tmp_path / "mean.npy"), np.load(tmp_path / "samples.npy")
    assert mean.shape == (8, 64 * 64) and samples.shape == (8, 64, 64 * 64)
    assert np.isfinite(mean).all() and np.isfinite(samples).all()
    full = run("--full", "--no-single-problem", "--no-full-loop", "--no-spmm", "--no-cpu-baseline")
    assert full["unit"] == "solves/s" and full["value"] > 0
    for k in ("roofline", "kernels", "phases_ms", "gemm_by_shape"):
        assert k in full, sorted(full)
    for k in ("single_problem", "full_loop", "roofline_spmm", "cpu_baseline", "parity"):
        assert k not in full, sorted(full)


def test_exact_variance_error_not_worse_than_lapack(pkg):
    """Why the exact-variance gate at darcy256 is cond-aware (7.5e-9 instead of BASELINE.md's flat 1e-9): entries of
    diag(Q^-1) in extended precision (columns Q^-1 e_i refined with long-double residuals, 24 interior nodes of the
    last eight blocks) -- the one-problem HIP path's selected inversion is no further from them than 2 x the oracle's."""
    from tests import measured_path as MP
    w = pkg.workloads.make("darcy256")
    Fo = O.tridiagonal_cholesky(w.Q, w.n_blocks)
    vo = O.marginal_variances_exact(Fo, last_blocks=8)
    F = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
    v = F.marginal_var("exact")
    rng = np.random.default_rng(17)
    cand = np.flatnonzero(vo > 50.0 * vo.min()) + (w.n - vo.size)
    idx = np.sort(rng.choice(cand, size=24, replace=False))
    vt = MP.true_inverse_diagonal(O, w.Q, Fo, idx)
    err_h = float(np.max(np.abs(v[idx] - vt) / vt))
    err_o = float(np.max(np.abs(vo[idx - (w.n - vo.size)] - vt) / vt))
    print(f"darcy256 exact variances vs extended precision: oracle {err_o:.2e}, HIP {err_h:.2e}")
    assert err_h <= 2.0 * err_o + 1e-13


def test_packed_transport_image_between_handles(pkg):
    """The unit a shared factor travels in (gmrf_bt_pack_blocks_async / _unpack_): lower-triangular 64 x 64 tiles of the
    block inverses, the stored windows of the coupling blocks, the blocks' log-determinant parts.  A batch of two
    darcy64 factors moves from one handle into another in two block ranges; the receiver (no L blocks, nothing factored)
    then solves, samples and reports log-determinants bitwise like the sender."""
    import torch
    w = pkg.workloads.make("darcy64")
    vals = np.stack([w.Q.data, 1.5 * w.Q.data])
    rhs = torch.from_numpy(np.stack([w.rhs, -w.rhs])[:, None, :]).cuda()
    F1 = pkg.TridiagonalCholeskyFactor(batch=2)
    F1.set_keep_l(False)
    F1.factor(w.Q, w.n_blocks, values=vals)
    F2 = pkg.TridiagonalCholeskyFactor(batch=2)
    F2.set_keep_l(False)
    F2.adopt_layout(w.n, w.n_blocks, F1.get_layout())
    N = w.n_blocks
    raw = 0
    for kind in (pkg._cabi.BLOCK_LINV, pkg._cabi.BLOCK_C):
        raw += F1.block_range(kind, 0, N)[1]
    packed = 0
    for i0, i1 in ((0, 5), (5, N)):
        sz = F1.packed_size(i0, i1)
        packed += sz
        buf = torch.full((2, sz), float("nan"), dtype=torch.float64, device="cuda")
        F1.pack_blocks_async(i0, i1, buf)
        F1.synchronize()
        F2.unpack_blocks_async(i0, i1, buf)
        F2.synchronize()
    nt = 256 // 64
    assert packed == N * (nt * (nt + 1) // 2) * 4096 + (F1.block_range(pkg._cabi.BLOCK_C, 0, N)[1]) + (2 + 6) + (2 + 12) and packed < 0.8 * raw    # (+ the 2-double representation tag per range)
    with pytest.raises(pkg.GmrfError):
        F2.solve_batch(rhs)                                  # not committed yet
    F2.adopt_commit(False)
    assert torch.equal(F1.solve_batch(rhs), F2.solve_batch(rhs))
    mu = F1.solve_batch(rhs)[:, 0, :]
    assert torch.equal(F1.sample_batch(8, mean=mu, seed=3, like=rhs), F2.sample_batch(8, mean=mu, seed=3, like=rhs))
    for p in (0, 1):
        F1.select_problem(p); F2.select_problem(p)
        assert F1.logdet() == F2.logdet()
    # a factor adopted as raw buffers (no transport image) has no log-determinant parts: loud, not garbage
    F3 = pkg.TridiagonalCholeskyFactor(batch=2)
    F3.set_keep_l(False)
    F3.adopt_layout(w.n, w.n_blocks, F1.get_layout())
    F3.adopt_commit(False)
    with pytest.raises(pkg.GmrfError):
        F3.logdet()
    # ... but a receiver that KEEPS L blocks and adopted the packed image without them reads the parts that travelled
    # (the keep_l branch used to refuse before looking at them)
    F4 = pkg.TridiagonalCholeskyFactor(batch=2)
    F4.adopt_layout(w.n, w.n_blocks, F1.get_layout())
    sz = F1.packed_size(0, N)
    buf = torch.empty((2, sz), dtype=torch.float64, device="cuda")
    F1.pack_blocks_async(0, N, buf); F1.synchronize()
    F4.unpack_blocks_async(0, N, buf); F4.synchronize()
    F4.adopt_commit(False)
    for p in (0, 1):
        F1.select_problem(p); F4.select_problem(p)
        assert F1.logdet() == F4.logdet()


def test_shallow_water_element_kernels_on_device(pkg):
    """SURVEY 8f rank 4, third piece: `assemble_system!` (/root/reference/src/spdes/shallow_water.jl:17-122) and the per-step
    operators of `discretize` (:170-217) on the device, entry by entry against the oracle's line-by-line restatement (fixed
    summation order: 1e-14 of the largest entry), with and without prescribed dofs, host and device-resident operands; then
    the initial precision Q_matern = J'J through the posterior assembler and the block-tridiagonal factor of it."""
    import torch
    for (nx, ny, kk, ff, gg, with_pres) in ((9, 7, 0.3, 0.7, 9.81, False), (40, 24, 0.0, 1e-4, 9.81, True), (96, 96, 0.05, 0.2, 1.0, True)):
        sw = pkg.ShallowWaterP1(nx, ny)
        qp = sw.qpoints
        H = 1.0 + 0.5 * np.sin(3.0 * qp[:, :, 0]) * np.cos(2.0 * qp[:, :, 1]) + 0.2 * qp[:, :, 0]
        nn = nx * ny
        pres = None
        if with_pres:                          # u and v prescribed on the boundary nodes (a wall), h free
            ixn, iyn = np.arange(nn) % nx, np.arange(nn) // nx
            bnd = (ixn == 0) | (iyn == 0) | (ixn == nx - 1) | (iyn == ny - 1)
            pres = np.zeros(3 * nn, dtype=bool); pres[1::3] = bnd; pres[2::3] = bnd
        Ko, Mo, So = O.assemble_shallow_water_system(nx, ny, H, kk, ff, gg, prescribed=pres)
        kv, ml, sv = sw.assemble(H, k=kk, f=ff, g=gg, prescribed=pres)
        # element sums in a fixed order: 1e-14 of the largest entry (measured <= 2e-15).  The diagonal entries of prescribed
        # dofs are meandiag, a sum over all 3 nn dofs that the device takes as a 256-way tree and NumPy pairwise: n eps at worst
        tol_e = 1e-14
        def close(dev, ora_data, pat):
            err = np.abs(dev - ora_data)
            big = np.max(np.abs(ora_data))
            if pres is None:
                print(f"shallow water {nx}x{ny}: max entry error {err.max() / big:.2e}")
                return err.max() < tol_e * big
            rows = np.repeat(np.arange(pat.shape[0]), np.diff(pat.indptr))
            md = (rows == pat.indices) & pres[rows]
            print(f"shallow water {nx}x{ny} constrained: entries {err[~md].max() / big:.2e}, meandiag {err[md].max() / big:.2e}")
            return err[~md].max() < tol_e * big and err[md].max() < 3 * nn * EPS * big
        assert close(kv, Ko.data, Ko) and close(sv, So.data, So)
        mdm = np.zeros(3 * nn, dtype=bool) if pres is None else pres
        assert np.max(np.abs(ml - Mo)[~mdm]) < tol_e * np.max(np.abs(Mo)) and np.max(np.abs(ml - Mo)) < 3 * nn * EPS * np.max(np.abs(Mo))
        tol = tol_e if pres is None else 3 * nn * EPS
        # device-resident operands give the same bits
        Hd = torch.from_numpy(H).cuda()
        pd = None if pres is None else torch.from_numpy(pres.astype(np.uint8)).cuda()
        kd, md, sd = sw.assemble(Hd, k=kk, f=ff, g=gg, prescribed=pd)
        assert kd.is_cuda and np.array_equal(kd.cpu().numpy(), kv) and np.array_equal(md.cpu().numpy(), ml) and np.array_equal(sd.cpu().numpy(), sv)
        oo = O.shallow_water_operators(Ko, Mo, So, pres, kappa_matern=3.0, tau=0.7, dt=0.05)
        od = sw.operators(kd, md, sd, prescribed=pd, kappa_matern=3.0, tau=0.7, dt=0.05)
        # (SciPy's sparse sums drop the explicit zeros the patterns keep: compare as matrices)
        Gd = sw.pattern_K.copy(); Gd.data = od["G_dt"].cpu().numpy()
        Jd = sw.pattern_S.copy(); Jd.data = od["J"].cpu().numpy()
        assert abs(Gd - oo["G_dt"]).max() < tol * abs(oo["G_dt"]).max()
        assert abs(Jd - oo["J"]).max() < 1e-13 * abs(oo["J"]).max()
        assert np.max(np.abs(od["M_tilde"].cpu().numpy() - oo["M_tilde"])) < 1e-15
        assert np.max(np.abs(od["beta"].cpu().numpy() - oo["beta"])) < 1e-15
    # the initial precision of the space-time model, Q_0 = J'J (:187), assembled on the device from J's values and factored
    # by the block-tridiagonal path (96 x 96 nodes x 3 fields, node-major: 4 node rows per block -> 24 blocks of 1152)
    J = Jd
    Z = sp.csc_matrix((3 * nn, 3 * nn))
    asm = pkg.PosteriorAssembler(Z, J)
    q0 = asm.precision(np.zeros(0), J.data, 1.0)
    Q0 = asm.pattern.copy(); Q0.data = np.asarray(q0)
    assert abs(Q0 - (oo["J"].T @ oo["J"])).max() < 1e-12 * abs(Q0).max()
    N = ny // 4
    F = pkg.tridiagonal_cholesky(Q0, N)
    b = np.random.default_rng(5).standard_normal(3 * nn)
    x = pkg.ldiv(F, b)
    qn = abs(Q0).sum(axis=1).max()
    assert np.linalg.norm(Q0 @ x - b) / (qn * np.linalg.norm(x) + np.linalg.norm(b)) < 1e-14
    assert rel(x, O.ldiv(O.tridiagonal_cholesky(Q0, N), b)) < 1e-9


def test_burgers_p2_tangent_on_device(pkg):
    """The Burgers residual and tangent on the QUADRATIC periodic line (the reference's element, src/utils.jl:42-49) on the
    device, entry by entry against the oracle's line-by-line restatement at three sizes, host and device-resident operands;
    then one Gauss-Newton style system Q + noise J'J assembled and factored (time-major: one block per time slice)."""
    import torch
    for ns, nt in ((12, 4), (64, 9), (512, 16)):
        dt, nu = 1.0 / (nt - 1), 0.01 / np.pi
        w = np.random.default_rng(ns).standard_normal(ns * nt)
        fo, Jo = O.burgers_f_and_J(ns, nt, dt, nu, w, order=2)
        b = pkg.BurgersP1Tangent(ns, nt, dt, nu, order=2)
        vals, f = b.tangent(w)
        assert np.array_equal(b.pattern.indices, Jo.indices)
        assert np.max(np.abs(vals - Jo.data)) < 1e-14 * np.max(np.abs(Jo.data))
        assert np.max(np.abs(f - fo)) < 1e-13 * np.max(np.abs(fo))
        vd, fd = b.tangent(torch.from_numpy(w).cuda())
        assert vd.is_cuda and np.array_equal(vd.cpu().numpy(), vals) and np.array_equal(fd.cpu().numpy(), f)
    # Q + noise J'J on the device and its block-tridiagonal factor (the coupling reaches one time slice)
    n = ns * nt
    Q = sp.identity(n, format="csc") * 1e-2
    asm = pkg.PosteriorAssembler(Q, b.pattern)
    a = asm.precision(Q.data, vals, 1e4)
    A = asm.pattern.copy(); A.data = np.asarray(a)
    Ao = (Q + 1e4 * (Jo.T @ Jo)).tocsc()
    assert abs(A - Ao).max() < 1e-13 * abs(Ao).max()
    F = pkg.tridiagonal_cholesky(A, nt)
    rhs = np.random.default_rng(1).standard_normal(n)
    x = pkg.ldiv(F, rhs)
    assert np.linalg.norm(A @ x - rhs) / (abs(A).sum(axis=1).max() * np.linalg.norm(x) + np.linalg.norm(rhs)) < 1e-14


def test_split_inverse_representation_of_batches(pkg):
    """Round 3: batches whose coupling blocks are zero left of column cmin >= 256 (darcy256: 256) do not assemble the
    first block column of Linv_i below row p = 256 -- C_i = B_i Linv_{i-1}^T never multiplies with it -- and keep the
    factor's own L[p:, 0:p] in its place; the sweeps apply X_aa, L_ba, X_bb one after the other.  Against the full
    representation (set_eager bit 12) on the leading 8 blocks of darcy256, batch 8, and against the oracle: same factor
    (log-determinants bitwise), means / samples / variances to rounding, fewer GEMM flops; Linv_i as a matrix
    (gmrf_bt_get_block) converts the factor to the full form; the layout record and the packed transport image carry the
    representation to another handle."""
    import torch
    w, vals_full, rhs_full = _darcy_batch(pkg, 256, 8)
    nb = 8
    ns = nb * w.block_size
    Q0 = w.Q.tocsr()[:ns, :ns].tocsc(); Q0.sort_indices()
    vals, rhs = [], []
    for p in range(8):
        Qp = w.Q.copy(); Qp.data = vals_full[p].copy()
        Qp = Qp.tocsr()[:ns, :ns].tocsc(); Qp.sort_indices()
        vals.append(Qp.data); rhs.append(rhs_full[p][:ns])
    vals, rhs = np.stack(vals), np.stack(rhs)
    rhs_t = torch.from_numpy(rhs[:, None, :]).cuda()
    Fs = pkg.TridiagonalCholeskyFactor(batch=8); Fs.set_keep_l(False)
    Ff = pkg.TridiagonalCholeskyFactor(batch=8); Ff.set_keep_l(False); Ff.set_eager(Switch.NO_XSPLIT)
    for F in (Fs, Ff):
        F.set_profiling(1)
        F.factor(Q0, nb, values=vals)
    assert Fs.get_layout()[-1] == 256 and Ff.get_layout()[-1] == 0
    fl = lambda F: sum(F.stats()["kernel_work"][c] for c in (13, 14, 15))
    assert fl(Fs) < 0.9 * fl(Ff)                               # the top doubling level does half the work, level 256 one pair less
    for F in (Fs, Ff):
        F.set_profiling(0)
    mu_s, mu_f = Fs.solve_batch(rhs_t)[:, 0, :], Ff.solve_batch(rhs_t)[:, 0, :]
    assert float((mu_s - mu_f).norm() / mu_f.norm()) < 1e-12
    Xs = Fs.sample_batch(64, mean=mu_s, seed=11, like=rhs_t)   # k = 64: the GEMM route of the sweeps
    Xf = Ff.sample_batch(64, mean=mu_s, seed=11, like=rhs_t)
    assert float((Xs - Xf).norm() / Xf.norm()) < 1e-12
    X16s = Fs.sample_batch(16, mean=mu_s, seed=11, like=rhs_t)  # k = 16: sweep_mm
    X16f = Ff.sample_batch(16, mean=mu_s, seed=11, like=rhs_t)
    assert float((X16s - X16f).norm() / X16f.norm()) < 1e-12
    for p in (0, 5):
        Fs.select_problem(p); Ff.select_problem(p)
        assert Fs.logdet() == Ff.logdet()
    # oracle, problem 5
    Q5 = Q0.copy(); Q5.data = vals[5].copy()
    Fo = O.tridiagonal_cholesky(Q5, nb)
    assert rel(mu_s[5].cpu().numpy(), O.ldiv(Fo, rhs[5])) < solve_tol(w)      # (bound of the full darcy256 posterior)
    # the receiving side of a shared factor: layout record + packed image, representation included
    Fr = pkg.TridiagonalCholeskyFactor(batch=8); Fr.set_keep_l(False)
    Fr.adopt_layout(ns, nb, Fs.get_layout())
    sz = Fs.packed_size(0, nb)
    buf = torch.empty((8, sz), dtype=torch.float64, device="cuda")
    Fs.pack_blocks_async(0, nb, buf); Fs.synchronize()
    Fr.unpack_blocks_async(0, nb, buf); Fr.synchronize()
    Fr.adopt_commit(False)
    assert Fr.get_layout()[-1] == 256
    assert torch.equal(Fr.solve_batch(rhs_t), Fs.solve_batch(rhs_t))
    # exact variances need Linv_i as a matrix: the factor converts itself (and says so in its layout record)
    vs, vf = Fs.marginal_var("exact"), Ff.marginal_var("exact")
    assert Fs.get_layout()[-1] == 0
    assert np.max(np.abs(vs - vf) / vf) < 1e-10
    Fs.select_problem(5); Ff.select_problem(5)
    Xi_s, Xi_f = Fs.get_block(pkg._cabi.BLOCK_LINV, 3), Ff.get_block(pkg._cabi.BLOCK_LINV, 3)
    assert np.max(np.abs(Xi_s - Xi_f)) < 1e-12 * np.max(np.abs(Xi_f))
    assert np.max(np.abs(Xi_s - np.linalg.inv(Fo.chos[3]))) < 1e-9 * np.max(np.abs(Xi_f))
    # sweeps after the conversion use the full form again and agree
    mu_c = Fs.solve_batch(rhs_t)[:, 0, :]
    assert float((mu_c - mu_f).norm() / mu_f.norm()) < 1e-12
    # Round 4: the layout record can be OLDER than the image -- the sender converted to the full form
    # (exact variances / get_block above) after the receiver fetched the record, and shares without re-factoring.
    # The packed image carries the representation its sender was in; the receiver's commit follows the image.
    stale_split = Fr.get_layout()                              # says 256; Fs now holds the FULL inverses
    assert stale_split[-1] == 256 and Fs.get_layout()[-1] == 0
    Fr.adopt_layout(ns, nb, stale_split)
    Fs.pack_blocks_async(0, nb, buf); Fs.synchronize()
    Fr.unpack_blocks_async(0, nb, buf); Fr.synchronize()
    Fr.adopt_commit(False)
    assert Fr.get_layout()[-1] == 0
    mu_r = Fr.solve_batch(rhs_t)[:, 0, :]
    assert torch.equal(mu_r, mu_c)
    assert float((mu_r - mu_f).norm() / mu_f.norm()) < 1e-12
    # the other order: the record was fetched while the sender was in the full form, the sender re-factors (split), shares
    stale_full = Fs.get_layout()
    assert stale_full[-1] == 0
    # re-factorisation returns to the split form
    Fs.refactor(vals)
    assert Fs.get_layout()[-1] == 256
    Fr.adopt_layout(ns, nb, stale_full)
    Fs.pack_blocks_async(0, nb, buf); Fs.synchronize()
    Fr.unpack_blocks_async(0, nb, buf); Fr.synchronize()
    Fr.adopt_commit(False)
    assert Fr.get_layout()[-1] == 256
    assert torch.equal(Fr.solve_batch(rhs_t), Fs.solve_batch(rhs_t))
    for F in (Fs, Ff, Fr):
        F.close()


def test_darcy_p2_triangle_stiffness_on_device(pkg):
    """Quadratic triangles: `assemble_darcy_diff_matrix` (/root/reference/src/problems/darcy.jl:5-63) with the reference's
    own element (Lagrange{RefTriangle,2}, QuadratureRule{RefTriangle}(3): src/utils.jl:32-33) on the device, entry by
    entry against the oracle's restatement (fixed summation order over a lattice point's cells and the quadrature
    points: 1e-14 of max |G|), host and device-resident operands; then the problem chain table -> G (device) ->
    Q + Q_eps G'G (device) -> block-tridiagonal factor -> mean against the oracle on the lattice (reach of G'G: four
    lattice rows = one block)."""
    import torch
    import scipy.sparse as sp
    gq = np.linspace(0.0, 1.0, 241)
    GX, GY = np.meshgrid(gq, gq, indexing="ij")
    for (nx, ny, seed) in ((9, 8, 523802340), (33, 33, 11), (128, 96, 7)):
        table = pkg.workloads.darcy_coefficient(seed)(GX.ravel(), GY.ravel()).reshape(241, 241)
        Go, fo = O.assemble_darcy_diff_matrix_p2(nx, ny, gq, gq, table, 2.0)
        d = pkg.DarcyP1Assembler(nx, ny, order=2)
        assert d.n == (2 * nx - 1) * (2 * ny - 1) and np.array_equal(d.pattern.indptr, Go.indptr) and np.array_equal(d.pattern.indices, Go.indices)
        vals, f = d.assemble(table, beta=2.0)
        ev, ef = np.max(np.abs(vals - Go.data)) / np.max(np.abs(Go.data)), np.max(np.abs(f - fo)) / np.max(np.abs(fo))
        print(f"darcy P2 {nx}x{ny}: entries {ev:.2e}, load {ef:.2e}")
        # (the boundary lattice points carry meandiag, an n-term sum taken as a 256-way tree here and pairwise by NumPy)
        W, H = 2 * nx - 1, 2 * ny - 1
        rows = np.repeat(np.arange(d.n), np.diff(Go.indptr))
        bnd = lambda r: (r % W == 0) | (r // W == 0) | (r % W == W - 1) | (r // W == H - 1)
        md = (rows == Go.indices) & bnd(rows)
        err = np.abs(vals - Go.data)
        assert err[~md].max() < 1e-14 * np.max(np.abs(Go.data)) and err[md].max() < d.n * EPS * np.max(np.abs(Go.data))
        assert ef < 1e-14
        vd, fd = d.assemble(torch.from_numpy(table).cuda(), beta=2.0)
        assert vd.is_cuda and np.array_equal(vd.cpu().numpy(), vals) and np.array_equal(fd.cpu().numpy(), f)
    # chain: 17 x 15 lattice (nx = 9, ny = 8), 3 blocks of 5 lattice rows
    nx, ny, N, q_eps = 9, 8, 3, 1e4
    d = pkg.DarcyP1Assembler(nx, ny, order=2)
    n = d.n
    Q0 = sp.identity(n, format="csc") * 2.0
    asm = pkg.PosteriorAssembler(Q0, d.pattern)
    table = pkg.workloads.darcy_coefficient(5)(GX.ravel(), GY.ravel()).reshape(241, 241)
    a_vals, y = d.assemble(torch.from_numpy(table).cuda())
    p_vals = asm.precision(torch.from_numpy(Q0.data).cuda(), a_vals, q_eps)
    P = asm.pattern.copy(); P.data = p_vals.cpu().numpy()
    F = pkg.tridiagonal_cholesky(P, N)
    rhs = asm.rhs(None, a_vals, torch.zeros(n, dtype=torch.float64, device="cuda"), y, q_eps)
    mu = pkg.ldiv(F, rhs)
    Go, fo = O.assemble_darcy_diff_matrix_p2(nx, ny, gq, gq, table, 1.0)
    _, _, mu_o = O.condition_on_observations(Q0, None, Go, q_eps, fo, N)
    assert rel(mu.cpu().numpy(), mu_o) < 1e-10
