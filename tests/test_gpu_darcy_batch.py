"""Batched device-resident conditioning for the Darcy data-set loop (gmrf_darcy_p1_assemble_batch, the batched RBMC / MC
estimators, gmrf_dc_run): every new piece against the existing call, or composition of existing calls, that it must
reproduce bit for bit, and against the oracle's restatement of the loop."""
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import bt_oracle as O
from tests.test_gpu_parity import EPS, rel, solve_tol

pytestmark = pytest.mark.gpu

Q_EPS = 1e8
NG = 241
GQ = np.linspace(0.0, 1.0, NG)
SEED0 = 523802340
_cache = {}


def coeff_tables(pkg, B, seed=SEED0):
    key = ("tab", B, seed)
    if key not in _cache:
        GX, GY = np.meshgrid(GQ, GQ, indexing="ij")
        _cache[key] = np.stack([pkg.workloads.darcy_coefficient(seed + p)(GX.ravel(), GY.ravel()).reshape(NG, NG) for p in range(B)])
    return _cache[key]


def prior(pkg, n_xy):
    key = ("prior", n_xy)
    if key not in _cache:
        Q0, _, N = pkg.workloads.darcy_conditioning(n_xy)
        _cache[key] = (Q0, N)
    return _cache[key]


def setup(pkg, n_xy, B, stream=None, eager=0):
    """Darcy assembler, posterior assembler and a batch-B handle factored once on the posterior pattern, on one stream.
    eager = Switch.BATCH_ROUTES: a one-problem handle runs the launch sequence of a batch (the bits of a batch's problem)."""
    import torch
    Q0, N = prior(pkg, n_xy)
    st = stream if stream is not None else torch.cuda.Stream()
    d = pkg.DarcyP1Assembler(n_xy, n_xy, stream=st.cuda_stream)
    asm = pkg.PosteriorAssembler(Q0, d.pattern, stream=st.cuda_stream)
    tabs = coeff_tables(pkg, B)
    td = torch.from_numpy(tabs).cuda()
    qd = torch.from_numpy(Q0.data).cuda()
    av, y = d.assemble_batch(td)
    nz = asm.precision_batch(qd, av, Q_EPS)
    F = pkg.TridiagonalCholeskyFactor(stream=st.cuda_stream, batch=B)
    if eager:
        F.set_eager(eager)
    P = asm.pattern.copy()
    P.data = nz[0].cpu().numpy().copy()
    F.factor(P, N, values=nz.cpu().numpy())
    return SimpleNamespace(Q0=Q0, N=N, n=n_xy * n_xy, st=st, d=d, asm=asm, F=F, P=P, tabs=tabs, td=td, qd=qd, av=av, y=y, nz=nz, B=B)


def composed(pkg, e, Q_mu, k_samples, k_var, sample_seed, var_seed):
    """The driver's work from the public calls that exist without it, on the same handle."""
    import torch
    av, y = e.d.assemble_batch(e.td)
    nz = e.asm.precision_batch(e.qd, av, Q_EPS)
    rhs = e.asm.rhs_batch(Q_mu, av, torch.zeros_like(y), y, Q_EPS)
    e.F.set_factor_rhs(rhs)
    e.F.refactor(nz)
    state = np.zeros(1, dtype=np.int32)
    pkg._cabi.check(pkg._cabi.load().gmrf_test_factor_fwd(e.F._h, pkg._cabi.ptr(state), None))
    mean, smp = e.F.posterior_batch(rhs, k_samples, seed=sample_seed)
    Pp = e.P.copy()
    Pp.data = nz[0].cpu().numpy().copy()
    Qc = pkg.CsrMatrix(Pp, stream=e.st.cuda_stream)
    var = torch.empty((e.n,) if e.B == 1 else (e.B, e.n), dtype=torch.float64, device="cuda")
    e.F.marginal_var("rbmc", k=k_var, seed=var_seed, Q=Qc, q_values=nz, out=var)
    e.F.set_factor_rhs(None)
    return mean, smp, torch.sqrt(var).reshape(e.B, e.n), int(state[0]), nz


def oracle_problem(e, n_xy, p, Q_mu=None):
    G, f = O.assemble_darcy_diff_matrix(n_xy, n_xy, GQ, GQ, e.tabs[p], 1.0)
    Qp, Fo, mu = O.condition_on_observations(e.Q0, None, G, Q_EPS, f, e.N)
    if Q_mu is not None:
        mu = O.ldiv(Fo, Q_mu + Q_EPS * (G.T @ f))
    return Qp, Fo, mu


@pytest.mark.parametrize("order,nx,ny", [(1, 12, 12), (2, 12, 12), (1, 9, 14)])
def test_assembly_batch_is_the_one_problem_call_bitwise(pkg, order, nx, ny):
    """B = 5 tables, host and device inputs: row p of `assemble_batch` is `assemble(tables[p])` bit for bit; problems 0 and 4
    against the oracle at the tolerances of the one-problem assembly tests (1e-14 of max |G|; the mean-diagonal entries of the
    quadratic element, an n-term sum, n eps).  9 x 14: a batch stride (nnz) that is no power of two."""
    import torch
    B = 5
    tabs = coeff_tables(pkg, B)
    d = pkg.DarcyP1Assembler(nx, ny, order=order)
    vb, fb = d.assemble_batch(tabs, beta=2.0)
    assert vb.shape == (B, d.nnz) and fb.shape == (B, d.n) and d.nnz & (d.nnz - 1) != 0
    vd, fd = d.assemble_batch(torch.from_numpy(tabs).cuda(), beta=2.0)
    assert vd.is_cuda and np.array_equal(vd.cpu().numpy(), vb) and np.array_equal(fd.cpu().numpy(), fb)
    for p in range(B):
        v1, f1 = d.assemble(tabs[p], beta=2.0)
        assert np.array_equal(vb[p], v1) and np.array_equal(fb[p], f1), p
    asm_o = O.assemble_darcy_diff_matrix if order == 1 else O.assemble_darcy_diff_matrix_p2
    for p in (0, 4):
        Go, fo = asm_o(nx, ny, GQ, GQ, tabs[p], 2.0)
        assert np.array_equal(d.pattern.indices, Go.indices)
        err, top = np.abs(vb[p] - Go.data), np.max(np.abs(Go.data))
        print(f"order {order} {nx}x{ny} problem {p}: entries {err.max() / top:.2e}, load {np.max(np.abs(fb[p] - fo)) / np.max(np.abs(fo)):.2e}")
        if order == 1:
            assert err.max() < 1e-14 * top
        else:
            W, H = 2 * nx - 1, 2 * ny - 1
            rows = np.repeat(np.arange(d.n), np.diff(Go.indptr))
            bnd = (rows % W == 0) | (rows // W == 0) | (rows % W == W - 1) | (rows // W == H - 1)
            md = (rows == Go.indices) & bnd
            assert err[~md].max() < 1e-14 * top and err[md].max() < d.n * EPS * top
        assert np.max(np.abs(fb[p] - fo)) < 1e-14 * np.max(np.abs(fo))


@pytest.mark.parametrize("order", [1, 2])
def test_one_darcy_assembler_serves_every_call_in_turn(pkg, order):
    """One assembler's batch and one-problem calls share its arena and its work buffer: batch of 3, table 1, batch of 3 again,
    table 2, with host arrays and with device tensors.  Every result is that of the same call on a fresh assembler, and each
    one-problem result is its row of the batch, bit for bit.  5 x 4 nodes, ng = 7: interior, edge and corner rows, a 2 x 2
    block of quadratic cells."""
    import torch
    nx, ny, ng = 5, 4, 7
    tabs = np.exp(np.random.default_rng(11).standard_normal((3, ng, ng)))
    host = lambda a: a.cpu().numpy() if torch.is_tensor(a) else a      # noqa: E731
    for kind, t in (("host", tabs), ("device", torch.from_numpy(tabs).cuda())):
        calls = [("assemble_batch", t), ("assemble", t[1]), ("assemble_batch", t), ("assemble", t[2])]
        d = pkg.DarcyP1Assembler(nx, ny, order=order)
        got = [[host(a) for a in getattr(d, name)(arg, beta=2.0)] for name, arg in calls]
        for i, (name, arg) in enumerate(calls):
            want = getattr(pkg.DarcyP1Assembler(nx, ny, order=order), name)(arg, beta=2.0)
            assert all(np.array_equal(g, host(w)) for g, w in zip(got[i], want)), (kind, i, name)
        for one, row in ((1, 1), (3, 2)):
            assert all(np.array_equal(g, b[row]) for g, b in zip(got[one], got[0])), (kind, row)


def _run_vs_composed(pkg, e, device_inputs):
    import torch
    rng = np.random.default_rng(4)
    Q_mu = rng.standard_normal((e.B, e.n))
    Q_mu_d = torch.from_numpy(Q_mu).cuda()
    mean, smp, std, state, nz = composed(pkg, e, Q_mu_d, 2, 50, 11, 13)
    dc = pkg.DarcyConditioningBatch(e.F, e.asm, e.d)
    if device_inputs:
        r = dc.run(e.td, e.qd, Q_mu=Q_mu_d, k_samples=2, var="rbmc", k_var=50, sample_seed=11, var_seed=13)
        assert r.mean.is_cuda and r.samples.is_cuda and r.std.is_cuda and r.std_norm.is_cuda
        got = [x.cpu().numpy() for x in (r.mean, r.samples, r.std, r.std_norm)]
    else:
        r = dc.run(e.tabs, e.Q0.data, Q_mu=Q_mu, k_samples=2, var="rbmc", k_var=50, sample_seed=11, var_seed=13)
        got = [r.mean, r.samples, r.std, r.std_norm]
    stats = e.F.stats()
    dc.close()
    assert got[1].shape == (e.B, 2, e.n)
    assert np.array_equal(got[0], mean.cpu().numpy())
    assert np.array_equal(got[1], smp.cpu().numpy())
    assert np.array_equal(got[2], std.cpu().numpy())
    ref = np.linalg.norm(got[2], axis=1)
    print("std_norm rel", np.max(np.abs(got[3] - ref) / ref))
    assert np.max(np.abs(got[3] - ref) / ref) < 1e-13
    return got, stats


def test_batch_of_one_takes_the_persistent_sweeps(pkg):
    """A batch of one goes through the abort-and-repeat guard of the persistent sweeps.  They need blocks of 512 .. 1024 and the
    whole chip (sweep_persist_demand), which darcy64's blocks of 256 do not give: darcy128 (32 blocks of 512), B = 1, while no
    other handle of this module is alive.  `run` is the composition bit for bit there too; stats(): the route was taken,
    nothing gave up."""
    e = setup(pkg, 128, 1)
    _, stats = _run_vs_composed(pkg, e, True)
    assert stats["sweep_persist"] == 1 and stats["persist_aborts"] == 0, stats
    e.F.close()


@pytest.fixture(scope="module")
def env5(pkg):
    return setup(pkg, 64, 5)


def _var_groups(pkg, F):
    size, groups = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    pkg._cabi.check(pkg._cabi.load().gmrf_test_var_groups(F._h, pkg._cabi.ptr(size), pkg._cabi.ptr(groups)))
    return int(size[0]), int(groups[0])


def _finish(acc, scale, base, fused):
    """base + acc * scale as the device's finish kernel rounds it: one rounding (fused) or two."""
    if not fused:
        return base + acc * scale
    s = Fraction(scale)
    return np.array([float(Fraction(a) * s + Fraction(b)) for a, b in zip(acc.tolist(), base.tolist())])


@pytest.mark.parametrize("method", ["rbmc", "mc"])
@pytest.mark.parametrize("k", [50, 70])
def test_batched_variances_are_the_one_problem_accumulation_bitwise(pkg, env5, monkeypatch, method, k):
    """darcy64, B = 5, k = 50 (one chunk, kcp = 50) and 70 (two chunks), the stage capped at 9 MB so that the problems go
    through it as 2 + 2 + 1 (a problem's stage is 3.3 MB at kcp = 50, 4.2 MB at 64; MC: half of that, capped at 4 MB; the
    grouping is read back with gmrf_test_var_groups): problem p's variances are, bit for bit,
    the finish of what a one-problem handle factored on p's values (set_eager bit 1: a batch's launch sequence) accumulates with first_id = p k (`var_accumulate`); the
    finish expression base + acc / k is rounded as the one-problem `marginal_var` rounds it (read off problem 0).  The default
    cap (one group) gives the same bits."""
    import torch
    e = env5
    monkeypatch.setenv("GMRF_VAR_STAGE_MB", "9" if method == "rbmc" else "4")      # (MC stages X alone: half of RBMC's X and Q X)
    e.F.refactor(e.nz)
    Qc = pkg.CsrMatrix(e.P, stream=e.st.cuda_stream)
    vb = e.F.marginal_var(method, k=k, seed=77, Q=Qc, q_values=e.nz)
    assert _var_groups(pkg, e.F) == (2, 3)                     # problems per group, groups: 2 + 2 + 1
    monkeypatch.delenv("GMRF_VAR_STAGE_MB")
    vb_one_group = e.F.marginal_var(method, k=k, seed=77, Q=Qc, q_values=e.nz, out=torch.empty((5, e.n), dtype=torch.float64, device="cuda"))
    assert _var_groups(pkg, e.F) == (5, 1)
    assert np.array_equal(vb_one_group.cpu().numpy(), vb)
    nz = e.nz.cpu().numpy()
    fused = None
    for p in range(5):
        Pp = e.P.copy()
        Pp.data = nz[p].copy()
        F1 = pkg.TridiagonalCholeskyFactor()
        F1.set_eager(pkg.Switch.BATCH_ROUTES)                                    # the launch sequence of a batch: its bits (test_batch_of_problems_matches_one_by_one)
        F1.factor(Pp, e.N)
        Q1 = pkg.CsrMatrix(Pp)
        acc = F1.var_accumulate(np.zeros(e.n), method, p * k, k, seed=77, Q=Q1 if method == "rbmc" else None)
        base = 1.0 / Pp.diagonal() if method == "rbmc" else np.zeros(e.n)
        if p == 0:
            v1 = F1.marginal_var(method, k=k, seed=77, Q=Q1 if method == "rbmc" else None)
            fused = np.array_equal(v1, _finish(acc, 1.0 / k, base, True))
            assert fused or np.array_equal(v1, _finish(acc, 1.0 / k, base, False))
            assert np.array_equal(vb[0], v1)
        assert np.array_equal(vb[p], _finish(acc, 1.0 / k, base, fused)), (p, method, k)
        F1.close()


def test_driver_is_the_composition_of_the_public_calls_bitwise(pkg):
    """darcy64, k_samples = 2, RBMC(50), non-zero Q mu: `run` gives the bits of assemble_batch -> precision_batch -> rhs_batch ->
    set_factor_rhs -> refactor -> posterior_batch -> marginal_var(rbmc, q_values) -> sqrt on the same handle, with host and
    with device arrays; std_norm is numpy.linalg.norm to 1e-13 and the same bits for problem 0 in a batch of 3 and of 1."""
    e3 = setup(pkg, 64, 3)
    got3, _ = _run_vs_composed(pkg, e3, False)
    got3d, _ = _run_vs_composed(pkg, e3, True)
    for a, b in zip(got3, got3d):
        assert np.array_equal(a, b)
    e1 = setup(pkg, 64, 1, eager=pkg.Switch.BATCH_ROUTES)
    got1, stats = _run_vs_composed(pkg, e1, True)
    assert stats["persist_aborts"] == 0, stats
    # problem 0 alone through a batch's launch sequence (set_eager bit 1): the same factor, so the same std, and the same norm
    assert np.array_equal(got1[2][0], got3[2][0]) and got1[3][0] == got3[3][0]
    e3.F.close(); e1.F.close()


@pytest.mark.parametrize("n_xy,B,want", [(64, 3, 0), (128, 16, 1)])
def test_both_solve_routes(pkg, n_xy, B, want):
    """The forward sweep inside the factorisation (gmrf_test_factor_fwd after the composed refactor on the same handle and shapes):
    and gmrf_test_dc_route for the driver's own): not taken at darcy64 with B = 3, taken at darcy128 (n = 16 384, 32 blocks of 512) with B = 16.  On both sides `run` gives
    the composed mean bit for bit, and the means of two problems agree with the oracle's `condition_on_observations`."""
    import torch
    e = setup(pkg, n_xy, B)
    zero = torch.zeros((B, e.n), dtype=torch.float64, device="cuda")
    mean, _, _, state, _ = composed(pkg, e, zero, 1, 8, 3, 5)
    assert state == want, state
    dc = pkg.DarcyConditioningBatch(e.F, e.asm, e.d)
    r = dc.run(e.td, e.qd, k_samples=1, var=None, sample_seed=3)
    route = np.zeros(1, dtype=np.int32)
    pkg._cabi.check(pkg._cabi.load().gmrf_test_dc_route(dc._h, pkg._cabi.ptr(route)))
    assert int(route[0]) == want                              # the driver's own factorisation, read before it put the registration back
    assert r.std is None and np.array_equal(r.mean.cpu().numpy(), mean.cpu().numpy())
    for p in (0, B - 1):
        Qp, _, mu_o = oracle_problem(e, n_xy, p)
        w = SimpleNamespace(Q=Qp, meta={})
        err = rel(r.mean[p].cpu().numpy(), mu_o)
        print(f"darcy{n_xy} B={B} problem {p}: mean rel {err:.2e} (tol {solve_tol(w):.2e})")
        assert err < solve_tol(w)
    dc.close(); e.F.close()


def test_run_against_the_oracle_end_to_end(pkg, env5):
    """darcy64, B = 5, problems 0 and 3: mean and samples (the device's normals fed to the oracle's `sample`) within solve_tol,
    the RBMC std against the oracle's estimator on the same draws at the RBMC parity test's 1e-8 (on the variances), the exact
    std at the exact-variance test's 1e-9."""
    e = env5
    dc = pkg.DarcyConditioningBatch(e.F, e.asm, e.d)
    k, kv = 2, 48
    r = dc.run(e.tabs, e.Q0.data, k_samples=k, var="rbmc", k_var=kv, sample_seed=21, var_seed=77)
    rx = dc.run(e.tabs, e.Q0.data, k_samples=0, var="exact")
    assert rx.samples is None and np.array_equal(rx.mean, r.mean)
    Z = e.F.normals_batch(k, seed=21)
    Zv = e.F.normals_batch(kv, seed=77)
    for p in (0, 3):
        Qp, Fo, mu_o = oracle_problem(e, 64, p)
        tol = solve_tol(SimpleNamespace(Q=Qp, meta={}))
        assert rel(r.mean[p], mu_o) < tol
        Xo = O.sample(Fo, mu_o, Z[p].T)
        assert rel(r.samples[p].T, Xo) < tol
        v_o = O.marginal_variances_rbmc(Qp, O.backward_solve(Fo, Zv[p].T))
        assert np.max(np.abs(r.std[p] ** 2 - v_o) / v_o) < 1e-8
        ve = O.marginal_variances_exact(Fo)
        assert np.max(np.abs(rx.std[p] ** 2 - ve) / ve) < 1e-9
        assert abs(rx.std_norm[p] - np.linalg.norm(rx.std[p])) < 1e-13 * rx.std_norm[p]
    dc.close()


def test_refusals_and_a_failed_factorisation(pkg, env5):
    """A twisted handle and a handle that analysed another pattern: GMRF_ERR_BAD_SHAPE.  An indefinite posterior raises
    NotPositiveDefinite naming the block, leaves the arrays passed in unchanged, and the next valid run on the same object
    gives the bits of a fresh object.  No coefficient table made the oracle's Cholesky fail (tried on the CPU at 16 x 16:
    a negative field, NaN in half the table, {1e10, 1e-10}, {1e14, 1}, {-1e14, 1} -- Q + q_eps A'A stays positive definite
    whatever A is); the indefinite posterior here is Q - 1e8 A'A, a negative q_eps on the valid tables, for which the oracle's
    Cholesky does fail."""
    e = env5
    cabi = pkg._cabi
    Ft = pkg.TridiagonalCholeskyFactor(stream=e.st.cuda_stream, order="twisted")
    with pytest.raises(pkg.GmrfError) as ex:
        pkg.DarcyConditioningBatch(Ft, e.asm, e.d)
    assert ex.value.status == cabi.ERR_BAD_SHAPE and "twisted" in str(ex.value)
    Ft.close()
    Fo = pkg.TridiagonalCholeskyFactor(stream=e.st.cuda_stream, batch=5)
    Fo.factor(e.Q0, e.N, values=np.tile(e.Q0.data, (5, 1)))               # the prior's pattern, not the posterior's
    with pytest.raises(pkg.GmrfError) as ex:
        pkg.DarcyConditioningBatch(Fo, e.asm, e.d).run(e.tabs, e.Q0.data)
    assert ex.value.status == cabi.ERR_BAD_SHAPE
    Fo.close()
    G, f = O.assemble_darcy_diff_matrix(64, 64, GQ, GQ, e.tabs[0], 1.0)
    with pytest.raises(O.NotPositiveDefinite):
        O.condition_on_observations(e.Q0, None, G, -Q_EPS, f, e.N)
    dc = pkg.DarcyConditioningBatch(e.F, e.asm, e.d)
    out = pkg.DarcyConditioningResult(np.full((5, e.n), 7.0), np.full((5, 1, e.n), 7.0), np.full((5, e.n), 7.0), np.full(5, 7.0))
    with pytest.raises(pkg.NotPositiveDefinite) as ex:
        dc.run(e.tabs, e.Q0.data, q_eps=-Q_EPS, out=out)
    assert 1 <= ex.value.info <= e.N and "block" in str(ex.value)
    assert all(np.all(a == 7.0) for a in (out.mean, out.samples, out.std, out.std_norm))
    for bad in (pkg.DarcyConditioningResult(np.zeros((5, e.n)), np.zeros((5, 1, e.n - 1)), np.zeros((5, e.n)), np.zeros(5)),
                pkg.DarcyConditioningResult(np.zeros((5, e.n)), np.zeros((5, 1, e.n)), np.zeros((4, e.n)), np.zeros(5)),
                pkg.DarcyConditioningResult(np.zeros((5, e.n), dtype=np.float32), np.zeros((5, 1, e.n)), np.zeros((5, e.n)), np.zeros(5))):
        with pytest.raises(ValueError):                        # arrays to fill are checked before the library writes into them
            dc.run(e.tabs, e.Q0.data, out=bad)
    r = dc.run(e.tabs, e.Q0.data)
    dc2 = pkg.DarcyConditioningBatch(e.F, e.asm, e.d)
    r2 = dc2.run(e.tabs, e.Q0.data)
    for a, b in ((r.mean, r2.mean), (r.samples, r2.samples), (r.std, r2.std), (r.std_norm, r2.std_norm)):
        assert np.array_equal(a, b)
    dc.close(); dc2.close()
