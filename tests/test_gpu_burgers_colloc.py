"""The Burgers collocation tangent on the device (gmrf_burgers_colloc_create behind the gmrf_burgers_p1_* calls) against
tests/burgers_colloc_oracle.py, and the batched Gauss-Newton loop bound to it on CO.COLLOC_CASE, compared one Gauss-Newton step at
a time: each step starts at the ORACLE's iterate, so differences do not accumulate along a trajectory."""
import numpy as np
import pytest

from tests import burgers_colloc_oracle as CO
from tests.test_gpu_parity import EPS, rel

pytestmark = pytest.mark.gpu

DT, NU = 0.05, 0.01
SHAPES = ((5, 3, 7), (20, 6, 27), (67, 5, 131))      # (nc, nt, npts): 14, 135 and 524 rows -- below, within and across 256-row workgroups


def smooth_plus_noise(ns, nt, seed):
    x, t = np.arange(ns) / ns, np.arange(nt)[:, None]
    return (np.sin(2 * np.pi * x)[None, :] * (1.0 - 0.1 * t) + 0.3 * np.cos(6 * np.pi * x + t) +
            0.1 * np.random.default_rng(seed).standard_normal((nt, ns))).ravel()


def step_tol(A):
    """The project's `solve_tol` rule (tests/test_gpu_parity.py) with the dense condition number of the step's matrix."""
    return max(1e-12, 0.25 * float(np.linalg.cond(A.toarray())) * EPS)


@pytest.fixture(scope="module")
def case(pkg):
    """COLLOC_CASE on the oracle, computed once and left unchanged: (workload, fJ, Qs, batch_loop result, tol), tol[k][p] the
    bound of problem p's step from iterate k (iterate 0 is the start point)."""
    c = CO.COLLOC_CASE
    w, fJ, Qs, res = CO.colloc_case(pkg.workloads)
    _, steps, _, _, its = res
    tol = []
    for k in range(int(steps.max())):
        xk = w["x0"] if k == 0 else its[k - 1]
        tol.append([step_tol(CO.posterior_matrix(Qs[p], fJ(xk[p])[1], w["noise"])) for p in range(c["B"])])
    return w, fJ, Qs, res, np.array(tol)


@pytest.mark.parametrize("nc,nt,npts", SHAPES)
def test_tangent_against_the_oracle_entry_by_entry(pkg, nc, nt, npts):
    B = 3
    pts = CO.special_points(nc, npts)
    b = pkg.BurgersCollocationTangent(nc, nt, DT, NU, pts)
    W = np.stack([smooth_plus_noise(b.ns, nt, 8 + p) for p in range(B)])
    vals, f = b.tangent_batch(W)
    assert vals.shape == (B, b.nnz) and f.shape == (B, b.rows)
    for p in range(B):
        fo, Jo = CO.f_and_J(nc, nt, DT, NU, pts, W[p])
        assert np.array_equal(b.pattern.indices, Jo.indices) and np.array_equal(b.pattern.indptr, Jo.indptr)
        ev, ef = np.max(np.abs(vals[p] - Jo.data)), np.max(np.abs(f[p] - fo))
        print(f"{nc}x{nt}x{npts} p={p}: max |J| {np.max(np.abs(Jo.data)):.3e} err {ev:.2e}; max |f| {np.max(np.abs(fo)):.3e} err {ef:.2e}")
        assert ev <= 1e-13 * np.max(np.abs(Jo.data))
        assert ef <= 1e-13 * max(np.max(np.abs(fo)), 1.0)
        assert np.array_equal(vals[p] == 0.0, Jo.data == 0.0) and np.any(vals[p] == 0.0)        # the stored zeros: points on vertices


def test_bits(pkg):
    """A batch row is the one-problem call, device tensors give the bits of host arrays, two problems differ, and a handle with
    the points in another order gives the same rows, permuted."""
    import torch
    nc, nt, npts, B = 67, 5, 131, 3
    pts = CO.special_points(nc, npts)
    b = pkg.BurgersCollocationTangent(nc, nt, DT, NU, pts)
    W = np.stack([smooth_plus_noise(b.ns, nt, 20 + p) for p in range(B)])
    vals, f = b.tangent_batch(W)
    vd, fd = b.tangent_batch(torch.from_numpy(W).cuda())
    assert vd.is_cuda and np.array_equal(vd.cpu().numpy(), vals) and np.array_equal(fd.cpu().numpy(), f)
    for p in range(B):
        v1, f1 = b.tangent(W[p])
        v1d, f1d = b.tangent(torch.from_numpy(W[p]).cuda())
        assert np.array_equal(v1, vals[p]) and np.array_equal(f1, f[p])
        assert np.array_equal(v1d.cpu().numpy(), vals[p]) and np.array_equal(f1d.cpu().numpy(), f[p])
    assert not np.array_equal(vals[0], vals[1]) and not np.array_equal(f[0], f[1])
    perm = np.random.default_rng(5).permutation(npts)
    b2 = pkg.BurgersCollocationTangent(nc, nt, DT, NU, pts[perm])
    v2, f2 = b2.tangent_batch(W)
    assert np.array_equal(v2.reshape(B, nt - 1, npts, 6), vals.reshape(B, nt - 1, npts, 6)[:, :, perm])
    assert np.array_equal(f2.reshape(B, nt - 1, npts), f.reshape(B, nt - 1, npts)[:, :, perm])
    assert np.array_equal(b2.pattern.indices.reshape(nt - 1, npts, 6), b.pattern.indices.reshape(nt - 1, npts, 6)[:, perm])


@pytest.mark.parametrize("nc,nt,npts", SHAPES[:2])
def test_device_tangent_is_the_derivative_of_its_residual(pkg, nc, nt, npts):
    """f is quadratic in w, so (f(w + e v) - f(w - e v)) / 2e = J(w) v up to rounding: the check of tests/test_burgers_colloc_cpu.py
    with the device's f and J."""
    import scipy.sparse as sp
    rng = np.random.default_rng(3)
    pts = CO.special_points(nc, npts)
    b = pkg.BurgersCollocationTangent(nc, nt, DT, NU, pts)
    w, eps = rng.standard_normal(b.n), 1e-3
    V = rng.standard_normal((3, b.n))
    vals, _ = b.tangent(w)
    J = sp.csr_matrix((vals, b.pattern.indices, b.pattern.indptr), shape=b.pattern.shape)
    _, F = b.tangent_batch(np.concatenate([w + eps * V, w - eps * V]))
    for i in range(3):
        jv = J @ V[i]
        err = np.max(np.abs((F[i] - F[3 + i]) / (2 * eps) - jv))
        print(f"{nc}x{nt}x{npts}: {err:.2e} of {np.max(np.abs(jv)):.2e}")
        assert err <= 1e-8 * np.max(np.abs(jv))


class Setup:
    """Handle, assembler and tangent on ONE stream, the handle factored once on the assembler's pattern (values at x0)."""

    def __init__(self, pkg, w):
        import torch
        self.torch, self.w = torch, w
        self.B, self.noise = w["x0"].shape[0], w["noise"]
        self.stream = torch.cuda.Stream()
        s = self.stream.cuda_stream
        self.tan = pkg.BurgersCollocationTangent(w["nc"], w["n_blocks"], w["dt"], w["nu"], w["points"], length=w["length"], stream=s)
        self.asm = pkg.PosteriorAssembler(w["Q"], self.tan.pattern, stream=s)
        self.F = pkg.TridiagonalCholeskyFactor(stream=s, batch=self.B)
        jv, _ = self.tan.tangent_batch(w["x0"])
        self.F.factor(self.asm.pattern, w["n_blocks"], values=self.asm.precision_batch(w["q_values"], jv, self.noise))

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def run(self, gn, max_steps, rtol, x0=None):
        w = self.w
        return gn.run(self.dev(w["q_values"]), self.dev(w["Qx_prior"]), self.dev(w["x_prior"]), self.dev(w["x0"] if x0 is None else x0),
                      noise=self.noise, rtol=rtol, max_steps=max_steps)

    def close(self, *drivers):
        """Destroys the drivers and the handle now: a handle holds its claim of the chip's CUs until it is destroyed, and the
        garbage collector may leave that to a later test module."""
        for d in drivers:
            d.close()
        self.F.close()


def whole_loop_tol(tol, steps, p):
    """100 x the largest per-step bound of the problem's own steps."""
    return 100.0 * float(np.max(tol[:int(steps[p]), p]))


def test_one_gauss_newton_step_at_a_time(pkg, case):
    """For k = 0 .. 3 the device loop starts at the oracle's iterate k with max_steps = 1 and is compared with the oracle's iterate
    k + 1: rel <= max(1e-12, 0.25 cond eps), cond the dense condition number of that step's Q + noise J'J (n = 240)."""
    c = CO.COLLOC_CASE
    w, _, _, (_, so, _, _, its), tol = case
    assert so.min() >= 4
    s = Setup(pkg, w)
    assert s.tan.n == w["n"] == 240 and s.tan.rows == w["m"] == 135
    gn = pkg.GaussNewtonBatch(s.F, s.asm, s.tan)
    for k in range(4):
        x, steps, hist = s.run(gn, 1, c["rtol"], x0=w["x0"] if k == 0 else its[k - 1])
        assert np.array_equal(steps, np.ones(c["B"], dtype=np.int32))
        assert np.all(np.isfinite(hist))
        for p in range(c["B"]):
            e = rel(x[p].cpu().numpy(), its[k][p])
            print(f"step {k} -> {k + 1} p={p}: rel {e:.2e} (bound {tol[k][p]:.2e})")
            assert e <= tol[k][p]
    s.close(gn)


def test_whole_loop_against_the_oracle(pkg, case):
    c = CO.COLLOC_CASE
    w, _, _, (xo, so, ho, _, _), tol = case
    s = Setup(pkg, w)
    gn = pkg.GaussNewtonBatch(s.F, s.asm, s.tan)
    x, steps, hist = s.run(gn, c["max_steps"], c["rtol"])
    print("steps", steps, "oracle", so)
    assert np.array_equal(steps, so)
    for p in range(c["B"]):
        assert np.all(np.isfinite(hist[p, :steps[p] + 1])) and np.all(np.isnan(hist[p, steps[p] + 1:]))
        e = rel(x[p].cpu().numpy(), xo[p])
        print(f"p={p}: final x rel {e:.2e} (bound {whole_loop_tol(tol, so, p):.2e}), objective {hist[p, steps[p]]:.6e} oracle {ho[p, so[p]]:.6e}")
        assert e <= whole_loop_tol(tol, so, p)
    s.close(gn)


def test_finalize_leaves_the_factor_at_the_final_iterate(pkg, case):
    """logdet of every problem against the oracle's factor (SuperLU) of Q + noise J'J at the device's final iterate to 1e-10
    relative; the exact marginal variances finite and positive."""
    c = CO.COLLOC_CASE
    w, fJ, Qs, _, _ = case
    s = Setup(pkg, w)
    gn = pkg.GaussNewtonBatch(s.F, s.asm, s.tan)
    x, _, _ = s.run(gn, c["max_steps"], c["rtol"])
    assert gn.finalize() is s.F
    x = x.cpu().numpy()
    for p in range(c["B"]):
        s.F.select_problem(p)
        ld, ldo = s.F.logdet(), CO.logdet(CO.posterior_matrix(Qs[p], fJ(x[p])[1], w["noise"]))
        print(f"p={p}: logdet device {ld:.15e} oracle {ldo:.15e}")
        assert abs(ld - ldo) <= 1e-10 * abs(ldo)
    var = s.F.marginal_var("exact")
    assert var.shape == (c["B"], w["n"]) and np.all(np.isfinite(var)) and np.all(var > 0.0)
    s.close(gn)


def test_the_chain_the_script_runs(pkg, case):
    """Prior and initial-condition stage on the device (BurgersLinePrior on the periodic quadratic line, BurgersInitialConditionBatch),
    then GaussNewtonBatch with the collocation tangent on the same handle and assembler: the step counts and the final x of the run
    that was fed the host-built prior, within the whole-loop bound."""
    c = CO.COLLOC_CASE
    w, _, _, (_, so, _, _, _), tol = case
    import torch
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    prior = pkg.BurgersLinePrior(c["nc"], c["nt"], w["dt"], c["nu"], order=2, bc="periodic", ic_noise=c["ic_noise"], stream=st)
    tan = pkg.BurgersCollocationTangent(c["nc"], c["nt"], w["dt"], c["nu"], w["points"], stream=st)
    asm = pkg.PosteriorAssembler(prior.pattern, tan.pattern, stream=st)
    F = pkg.TridiagonalCholeskyFactor(stream=st, batch=c["B"])
    v = prior.values_batch(w["ic"])
    x_start = np.repeat(v["bulk"][:, None], w["n"], axis=1)
    x_start[:, :w["ns"]] = w["ic"]
    jv, _ = tan.tangent_batch(x_start)
    F.factor(asm.pattern, c["nt"], values=asm.precision_batch(v["q_values"], jv, w["noise"]))
    ic_stage = pkg.BurgersInitialConditionBatch(F, asm, prior)
    gn = pkg.GaussNewtonBatch(F, asm, tan)
    x_ic, q, qx, bulk = ic_stage.run(torch.from_numpy(w["ic"]).cuda())
    assert x_ic.is_cuda and q.is_cuda and qx.is_cuda
    x, steps, _ = gn.run(q, qx, x_ic, x_ic, noise=w["noise"], rtol=c["rtol"], max_steps=c["max_steps"])
    hs = Setup(pkg, w)
    gn_host = pkg.GaussNewtonBatch(hs.F, hs.asm, hs.tan)
    xh, steps_host, _ = hs.run(gn_host, c["max_steps"], c["rtol"])
    print("steps", steps, "on the host-built prior", steps_host, "oracle", so)
    assert np.array_equal(steps, steps_host)
    for p in range(c["B"]):
        e_ic, e = rel(x_ic[p].cpu().numpy(), w["x_prior"][p]), rel(x[p].cpu().numpy(), xh[p].cpu().numpy())
        print(f"p={p}: x_ic against the workload's {e_ic:.2e}; final x against the host-fed run {e:.2e} (bound {whole_loop_tol(tol, so, p):.2e})")
        assert e <= whole_loop_tol(tol, so, p)
    torch.cuda.synchronize()
    hs.close(gn_host)
    gn.close(); ic_stage.close(); F.close()
