"""The posterior stage of the batched Gauss-Newton loops on the device: gmrf_bt_logdet_batch, gmrf_assemble_quadform_batch and
gmrf_gn_posterior against the public calls they are made of (bitwise) and against tests/gn_posterior_oracle.py (derived bounds).

Measured on an MI355X (every figure printed by the tests, `-s`): see DESIGN section 5q."""
import ctypes as C
import math
import types

import numpy as np
import pytest

from oracle import bt_oracle as O
from tests import burgers_colloc_oracle as CO
from tests import elliptic_oracle as EO
from tests import gn_batch_oracle as GO
from tests import gn_posterior_oracle as PO
from tests.test_gpu_burgers_colloc import Setup as CollocSetup
from tests.test_gpu_elliptic import Setup as EllipticSetup
from tests.test_gpu_gn_batch import Setup
from tests.test_gpu_parity import rel, solve_tol

pytestmark = pytest.mark.gpu

FIELDS = ("samples", "std", "std_norm", "logdet", "sqmahal", "nll", "errors")
LOG_2PI = math.log(2.0 * math.pi)


def smooth(ns, nt, B):
    """(B, n) smooth fields of size 1: the perturbation of the scores' z."""
    xs, t = np.arange(ns) / ns, np.arange(nt)[:, None]
    return np.stack([(np.sin(2 * np.pi * (p + 1) * xs)[None, :] * np.cos(0.3 * t + p)).ravel() for p in range(B)])


def host(a):
    return a if a is None or isinstance(a, np.ndarray) else a.cpu().numpy()


class Ran:
    """GO.GN_CASE after its run, kept for the module: the setup, the driver, the final iterates and z = x + 1e-3 smooth."""

    def __init__(self, pkg):
        c = GO.GN_CASE
        self.c = c
        self.s = Setup(pkg, c["ns"], c["nt"], c["B"], seed=c["seed"])
        self.gn = pkg.GaussNewtonBatch(self.s.F, self.s.asm, self.s.tan)
        self.x, self.steps, self.hist = self.s.run(self.gn, c["max_steps"], c["rtol"])
        self.z = self.x + 1e-3 * smooth(c["ns"], c["nt"], c["B"])

    def values(self):
        """The posterior values at the final iterate through the public calls (device)."""
        s = self.s
        jv, _ = s.tan.tangent_batch(s.dev(self.x))
        return s.asm.precision_batch(s.dev(s.w["q_values"]), jv, s.noise)


@pytest.fixture(scope="module")
def ran(pkg):
    r = Ran(pkg)
    yield r
    r.gn.close()
    r.s.F.close()


def refused(pkg, fn, status):
    with pytest.raises(pkg.GmrfError) as e:
        fn()
    assert e.value.status == status


def test_logdet_batch_is_bitwise_the_selected_logdet(pkg, ran):
    """After finalize(), with and without resident L blocks, host and device `out`; a handle of N = 2 blocks; the refusals."""
    import torch
    s, B = ran.s, ran.c["B"]
    cabi = pkg._cabi
    for keep in (False, True):
        s.F.set_keep_l(keep)                                  # (a change of the flag drops the factor)
        refused(pkg, s.F.logdet_batch, cabi.ERR_NO_FACTOR)
        ran.gn.finalize()
        got = s.F.logdet_batch()
        got_dev = s.F.logdet_batch(out=torch.full((B,), 7.0, dtype=torch.float64, device="cuda"))
        assert got.shape == (B,) and np.array_equal(got_dev.cpu().numpy(), got)
        for p in range(B):
            s.F.select_problem(p)
            one = s.F.logdet()
            print(f"keep_l={keep} p={p}: {got[p]:.17e} {one:.17e}")
            assert one == got[p]
        assert len(set(got.tolist())) == B
        assert np.array_equal(s.F.logdet_batch(), got)
    s.F.select_problem(0)
    # two blocks, three problems
    w = pkg.workloads.random_block_tridiagonal(2, 40, seed=4)
    F2 = pkg.TridiagonalCholeskyFactor(batch=3)
    F2.factor(w.Q, 2, values=np.stack([w.Q.data * (1.0 + 0.25 * p) for p in range(3)]))
    got = F2.logdet_batch()
    for p in range(3):
        F2.select_problem(p)
        assert F2.logdet() == got[p]
        ref = np.linalg.slogdet(w.Q.toarray() * (1.0 + 0.25 * p))[1]
        assert abs(got[p] - ref) <= 1e-12 * abs(ref)
    with pytest.raises(ValueError):
        F2.logdet_batch(out=np.zeros(4))
    F2.close()
    Ft = pkg.TridiagonalCholeskyFactor(order="twisted")
    refused(pkg, Ft.logdet_batch, cabi.ERR_BAD_SHAPE)
    Ft.close()


def test_quadform_batch_against_the_longdouble_oracle(pkg):
    """ns = 72, nt = 30: n = 2160, two chunks of 1080 columns with the partition of std_norm_part, a thread's run ends mid-stride
    (1080 = 4 x 256 + 56).  B = 3, random x and z, the values of precision_batch at noise 1e12: every problem within
    depth eps |d|'|A||d| of the longdouble value, shared and per-problem values, host and device operands; problem p's bits at
    B = 3 are those of a B = 1 call on its slice, and two calls give the same bits."""
    import torch
    ns, nt, B, noise = 72, 30, 3, 1e12
    w = pkg.workloads.burgers_gauss_newton_batch(ns, nt, B, seed=2)
    tan = pkg.BurgersP1Tangent(ns, nt, w["dt"], w["nu"])
    asm = pkg.PosteriorAssembler(w["Q"], tan.pattern)
    assert asm.n == 2160 and PO.chunks(asm.n) == (2, 1080)
    assert len(set(np.diff(asm.pattern.indptr).tolist())) >= 2            # columns of unequal length
    jv, _ = tan.tangent_batch(w["x0"])
    vals = asm.precision_batch(w["q_values"], jv, noise)
    rng = np.random.default_rng(17)
    x, z = rng.standard_normal((B, asm.n)), rng.standard_normal((B, asm.n))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    for a_vals, per_problem in ((vals, True), (vals[1], False)):
        got = asm.quadform_batch(a_vals, x, z)
        assert got.shape == (B,) and np.array_equal(got, asm.quadform_batch(a_vals, x, z))
        got_dev = asm.quadform_batch(dev(a_vals), dev(x), dev(z))
        assert got_dev.is_cuda and np.array_equal(got_dev.cpu().numpy(), got)
        for p in range(B):
            A = GO.problem_matrix(asm.pattern, a_vals[p] if per_problem else a_vals)
            exact, bound = PO.sqmahal(A, x[p], z[p]), PO.quadform_bound(A, x[p], z[p])
            err = abs(float(PO.LD(got[p]) - exact))
            print(f"per_problem={per_problem} p={p}: device {got[p]:.17e} err {err:.3e} bound {bound:.3e} (depth {PO.depth(A)})")
            assert err <= bound
            one = asm.quadform_batch(a_vals[p:p + 1] if per_problem else a_vals, x[p:p + 1], z[p:p + 1])
            assert np.array_equal(one, got[p:p + 1])
    assert asm.quadform_batch(vals, x, x).tolist() == [0.0] * B
    with pytest.raises(ValueError):
        asm.quadform_batch(vals[:, :-1], x, z)


def _composed(pkg, ran, z, var, k_var, first, device):
    """The stage's results from the public calls, one after the other, on the same handle."""
    import torch
    s, c = ran.s, ran.c
    F = ran.gn.finalize()
    xd, zd = s.dev(ran.x), s.dev(z)
    smp = F.sample_batch(3, mean=xd, seed=21)
    values = ran.values()
    if var == "rbmc":
        P = s.asm.pattern.copy()
        P.data = values[0].cpu().numpy().copy()
        Qc = pkg.CsrMatrix(P, stream=s.stream.cuda_stream)
        v = F.marginal_var("rbmc", k=k_var, seed=77, Q=Qc, q_values=values,
                           out=torch.empty((c["B"], s.asm.n), dtype=torch.float64, device="cuda"))
    elif var == "exact":
        v = F.marginal_var("exact", out=torch.empty((c["B"], s.asm.n), dtype=torch.float64, device="cuda"))
    else:
        v = None
    std = None if v is None else torch.sqrt(v)
    ld = F.logdet_batch()
    sq = s.asm.quadform_batch(values, xd, zd)
    if device:
        err = pkg.solution_errors_batch(xd, zd, first=first)
    else:
        err = pkg.solution_errors_batch(ran.x, z, first=first)
    return host(smp), host(std), ld, host(sq), err


@pytest.mark.parametrize("var", ["rbmc", "exact", None])
def test_stage_is_the_composition_of_the_public_calls_bitwise(pkg, ran, var):
    """GO.GN_CASE, k_samples = 3: finalize -> sample_batch(3, mean = x) -> marginal_var on the assembled values -> sqrt ->
    logdet_batch -> quadform_batch -> solution_errors_batch, with torch and with NumPy inputs.  nll is the stated expression on
    those two scores, bit for bit; std_norm is numpy.linalg.norm to 1e-13 (another summation order)."""
    import torch
    c, s = ran.c, ran.s
    B, n, first = c["B"], s.asm.n, c["ns"]
    for device in (True, False):
        z = s.dev(ran.z) if device else ran.z
        r = ran.gn.posterior(z=z, first=first, k_samples=3, var=var, k_var=8, sample_seed=21, var_seed=77)
        assert all((getattr(r, f) is None or (torch.is_tensor(getattr(r, f)) and getattr(r, f).is_cuda)) if device
                   else (getattr(r, f) is None or isinstance(getattr(r, f), np.ndarray)) for f in FIELDS)
        assert np.array_equal(host(r.x), ran.x)
        smp, std, ld, sq, err = _composed(pkg, ran, ran.z, var, 8, first, device)
        assert r.samples.shape == (B, 3, n) and np.array_equal(host(r.samples), smp)
        if var is None:
            assert r.std is None and r.std_norm is None
        else:
            assert np.array_equal(host(r.std), std)
            nrm = host(r.std_norm)
            for p in range(B):
                assert abs(nrm[p] - np.linalg.norm(std[p])) <= 1e-13 * nrm[p]
        assert np.array_equal(host(r.logdet), ld) and np.array_equal(host(r.sqmahal), sq) and np.array_equal(host(r.errors), err)
        nll = 0.5 * ((n * LOG_2PI + sq) - ld)
        print(f"var={var} device={device}: logdet {ld[0]:.15e} sqmahal {sq[0]:.15e} nll {host(r.nll)[0]:.15e} errors {err[0]}")
        assert np.array_equal(host(r.nll), nll)
    # without z: no scores but logdet; arrays to fill are checked before the library writes into them
    r0 = ran.gn.posterior(k_samples=0, var=None)
    assert r0.samples is None and r0.sqmahal is None and r0.nll is None and r0.errors is None and np.array_equal(host(r0.logdet), ld)
    with pytest.raises(ValueError):
        ran.gn.posterior(out=pkg.GaussNewtonPosterior(sqmahal=np.zeros(B)), k_samples=0, var=None)
    with pytest.raises(ValueError):
        ran.gn.posterior(z=ran.z, out=pkg.GaussNewtonPosterior(errors=np.zeros((B, 2))), k_samples=0, var=None)
    with pytest.raises(ValueError):
        ran.gn.posterior(var="selinv")


def test_stage_against_the_oracle(pkg, ran):
    """GO.GN_CASE, problems 0 and 3, A = Q + noise J'J of the oracle at the device's final x: logdet to 1e-10 relative (the gate
    of test_finalize_leaves_the_factor_at_the_final_iterate), sqmahal within PO.stage_bound (z = x + 1e-3 smooth), nll within
    half the sum of the two, the device's normals through the oracle's `sample` within solve_tol, the exact std against the
    oracle's selected inverse at the exact-variance test's 1e-9 (on the variances), errors against workloads.solution_errors
    to 1e-13."""
    c, s = ran.c, ran.s
    w, ns, nt, n = s.w, c["ns"], c["nt"], s.asm.n
    r = ran.gn.posterior(z=ran.z, first=ns, k_samples=3, var="exact", sample_seed=21)
    Z = s.F.normals_batch(3, seed=21)
    for p in (0, 3):
        Qp = GO.problem_matrix(w["Q"], w["q_values"][p])
        _, J = O.burgers_f_and_J(ns, nt, w["dt"], w["nu"], ran.x[p])
        A = O.assemble_posterior(Qp, J, w["noise"])
        Fo = O.tridiagonal_cholesky(A, nt)
        ld_o = O.logdet(Fo)
        e_ld = abs(r.logdet[p] - ld_o)
        sq_o, b_sq = PO.sqmahal(A, ran.x[p], ran.z[p]), PO.stage_bound(Qp, J, w["noise"], ran.x[p], ran.z[p], 1e-14)
        e_sq = abs(float(PO.LD(r.sqmahal[p]) - sq_o))
        nll_o = PO.nll(A, ran.x[p], ran.z[p], logdet=ld_o)
        e_nll = abs(float(PO.LD(r.nll[p]) - nll_o))
        print(f"p={p}: logdet {r.logdet[p]:.15e} err {e_ld:.2e} (gate {1e-10 * abs(ld_o):.2e}); sqmahal {r.sqmahal[p]:.15e} err {e_sq:.2e} "
              f"(bound {b_sq:.2e}); nll {r.nll[p]:.15e} err {e_nll:.2e}")
        assert e_ld <= 1e-10 * abs(ld_o)
        assert e_sq <= b_sq
        assert e_nll <= 0.5 * (b_sq + 1e-10 * abs(ld_o))
        tol = solve_tol(types.SimpleNamespace(Q=A, meta={}))
        Xo = O.sample(Fo, ran.x[p], Z[p].T)
        assert rel(r.samples[p].T, Xo) < tol
        ve = O.marginal_variances_exact(Fo)
        assert np.max(np.abs(r.std[p] ** 2 - ve) / ve) < 1e-9
        assert abs(r.std_norm[p] - np.linalg.norm(r.std[p])) <= 1e-13 * r.std_norm[p]
        eo = pkg.workloads.solution_errors(ran.x[p][ns:], ran.z[p][ns:])
        for k, name in enumerate(("rel_err", "rmse", "max_err")):
            assert abs(r.errors[p, k] - eo[name]) <= 1e-13 * eo[name]


def _scores_against(pkg, r, x, z, mats, j_rel, logdet):
    for p, (Qp, J, noise) in enumerate(mats):
        A = CO.posterior_matrix(Qp, J, noise)
        ld_o = logdet(A)
        e_ld = abs(r.logdet[p] - ld_o)
        sq_o, b_sq = PO.sqmahal(A, x[p], z[p]), PO.stage_bound(Qp, J, noise, x[p], z[p], j_rel)
        e_sq = abs(float(PO.LD(r.sqmahal[p]) - sq_o))
        e_nll = abs(float(PO.LD(r.nll[p]) - PO.nll(A, x[p], z[p], logdet=ld_o)))
        print(f"p={p}: logdet {r.logdet[p]:.15e} err {e_ld:.2e}; sqmahal {r.sqmahal[p]:.15e} err {e_sq:.2e} (bound {b_sq:.2e}); nll err {e_nll:.2e}")
        assert e_ld <= 1e-10 * abs(ld_o)
        assert e_sq <= b_sq
        assert e_nll <= 0.5 * (b_sq + 1e-10 * abs(ld_o))


def test_collocation_tangent_where_m_is_not_n(pkg):
    """BurgersCollocationTangent(20, 6, 27 points) in the mild regime of CO.COLLOC_CASE, B = 2: m = 135, n = 240."""
    c = CO.COLLOC_CASE
    w, fJ, Qs, _ = CO.colloc_case(pkg.workloads, B=2, max_steps=0)
    s = CollocSetup(pkg, w)
    assert s.tan.rows == 135 and s.tan.n == 240
    gn = pkg.GaussNewtonBatch(s.F, s.asm, s.tan)
    x, steps, _ = s.run(gn, c["max_steps"], c["rtol"])
    x = x.cpu().numpy()
    z = x + 1e-3 * smooth(w["ns"], c["nt"], 2)
    r = gn.posterior(z=z, first=w["ns"], k_samples=1, var="rbmc", k_var=8)
    assert r.samples.shape == (2, 1, 240) and np.all(np.isfinite(r.samples)) and np.all(r.std > 0.0)
    _scores_against(pkg, r, x, z, [(Qs[p], fJ(x[p])[1], w["noise"]) for p in range(2)], 1e-13, CO.logdet)
    s.close(gn)


def test_elliptic_tangent(pkg):
    """EllipticP1Tangent on the 16 x 16 mesh, B = 2, y = tan.load(src_q), noise 3e13; z = the true solutions."""
    c = EO.GN_CASE
    w = pkg.workloads.elliptic_gauss_newton_batch((16, 16), 2, rows_per_block=c["rows_per_block"], amps=(0.5, 1.0))
    assert w["noise"] == 3e13
    prob = EO.Problem(w["nx"], w["ny"], w["src_q"])
    s = EllipticSetup(pkg, w)
    gn = pkg.GaussNewtonBatch(s.F, s.asm, s.tan)
    x, steps, _ = s.run(gn, c["max_steps"], c["rtol"])
    z = w["truth"]
    r = gn.posterior(z=z, k_samples=1, var="exact")
    for p in range(2):
        eo = pkg.workloads.solution_errors(x[p], z[p])
        assert abs(r.errors[p, 0] - eo["rel_err"]) <= 1e-13 * eo["rel_err"]
    logdet = lambda A: O.logdet(O.tridiagonal_cholesky(A, w["n_blocks"]))      # noqa: E731
    _scores_against(pkg, r, x, z, [(w["Q"], prob.fJ(p)(x[p])[1], w["noise"]) for p in range(2)], 1e-14, logdet)
    gn.close()
    s.F.close()


def test_refusals_and_a_failed_factorisation(pkg):
    """Before any run and after a run on another batch size: GMRF_ERR_NO_FACTOR.  An indefinite posterior (the sign of the noise,
    as the Darcy driver's test builds it) raises NotPositiveDefinite naming the block and leaves the arrays passed in unchanged;
    the next valid run and stage on the same objects give the bits of the stage before."""
    cabi = pkg._cabi
    c = GO.GN_CASE
    B, ns, nt = 3, c["ns"], c["nt"]
    s = Setup(pkg, ns, nt, B, seed=c["seed"])
    n = s.asm.n
    gn = pkg.GaussNewtonBatch(s.F, s.asm, s.tan)
    refused(pkg, gn.posterior, cabi.ERR_NO_FACTOR)
    x, _, _ = s.run(gn, 2, c["rtol"])
    z = x + 1e-3 * smooth(ns, nt, B)
    good = gn.posterior(z=z, k_samples=1, var="exact")
    s.F.set_batch(B + 1)
    refused(pkg, lambda: gn.posterior(k_samples=0, var=None), cabi.ERR_NO_FACTOR)
    s.F.set_batch(B)
    s.F.factor(s.asm.pattern, nt, values=s.values0)
    s.noise = -s.noise
    s.run(gn, 0, c["rtol"])                                      # (no iteration: the run only leaves its start point and its noise)
    s.noise = -s.noise
    out = pkg.GaussNewtonPosterior(None, np.full((B, 1, n), 7.0), np.full((B, n), 7.0), np.full(B, 7.0), np.full(B, 7.0), np.full(B, 7.0),
                                   np.full(B, 7.0), np.full((B, 3), 7.0))
    with pytest.raises(pkg.NotPositiveDefinite) as ex:
        gn.posterior(z=z, k_samples=1, var="exact", out=out)
    assert 1 <= ex.value.info <= nt and "block" in str(ex.value)
    assert all(np.all(getattr(out, f) == 7.0) for f in FIELDS)
    s.run(gn, 2, c["rtol"])
    again = gn.posterior(z=z, k_samples=1, var="exact")
    for f in FIELDS:
        assert np.array_equal(getattr(again, f), getattr(good, f)), f
    gn.close()
    s.F.close()


def test_neighbouring_calls_are_unchanged(pkg, ran):
    """A run after a stage gives the bits of the run before it; the stage's factorisation sees the caller's registered
    right-hand side and leaves it registered (burgers512x64 as a batch of 16, where the forward-in-factor route qualifies)."""
    c, s = ran.c, ran.s
    ran.gn.posterior(z=ran.z, k_samples=3, var="rbmc", k_var=8)
    x, steps, hist = s.run(ran.gn, c["max_steps"], c["rtol"])
    assert np.array_equal(x, ran.x) and np.array_equal(steps, ran.steps) and np.array_equal(hist, ran.hist, equal_nan=True)
    big = Setup(pkg, 512, 64, 16)
    gn = pkg.GaussNewtonBatch(big.F, big.asm, big.tan)
    big.run(gn, 1, 1e-4)
    probe = big.dev(big.w["Qx_prior"])
    big.F.set_factor_rhs(probe)
    state = C.c_int32(0)
    r = gn.posterior(k_samples=0, var=None)
    pkg._cabi.check(pkg._cabi.load().gmrf_test_factor_fwd(big.F._h, C.byref(state), None))
    assert state.value == 1 and np.all(np.isfinite(host(r.logdet)))
    big.F.set_factor_rhs(None)
    gn.close()
    big.F.close()
