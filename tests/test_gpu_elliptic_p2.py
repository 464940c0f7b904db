"""The quadratic-triangle elliptic tangent (gmrf_elliptic_p2_create behind the gmrf_elliptic_p1_* calls) and the batched
device-resident Gauss-Newton loop bound to it, against tests/elliptic_p2_oracle.py and against the one-problem device loop
(`gn_step`).  The shape of tests/test_gpu_elliptic.py, with its tolerances."""
import ctypes as C
import types

import numpy as np
import pytest
import scipy.sparse as sp

from tests import elliptic_oracle as EO
from tests import elliptic_p2_oracle as PO
from tests import gn_batch_oracle as GO
from tests.test_gpu_parity import rel, solve_tol

pytestmark = pytest.mark.gpu

# vertices per side: (2, 2) one interior dof, a diagonal midpoint; (3, 3) every dof class, one interior vertex with six cells;
# (8, 8) 225 rows; (10, 8) 285 rows: non-square, two workgroups, the last one partial
MESHES = ((2, 2), (3, 3), (8, 8), (10, 8))


@pytest.fixture(scope="module")
def gn_cases(pkg):
    """PO.GN_CASE_P2 on both meshes, computed once and left unchanged: mesh -> (workload, Problem, batch_loop result)."""
    return {ms: PO.oracle_case(pkg.workloads, ms) for ms in PO.GN_CASE_P2["meshes"]}


class Setup:
    """Handle, assembler and tangent on ONE stream, the handle factored once on the assembler's pattern (values at x0)."""

    def __init__(self, pkg, w):
        import torch
        self.torch, self.w = torch, w
        self.B, self.noise = w["x0"].shape[0], w["noise"]
        self.stream = torch.cuda.Stream()
        s = self.stream.cuda_stream
        self.tan = pkg.EllipticP1Tangent(w["nx"], w["ny"], stream=s, order=w.get("order", 1))
        self.asm = pkg.PosteriorAssembler(w["Q"], self.tan.pattern, stream=s)
        self.F = pkg.TridiagonalCholeskyFactor(stream=s, batch=self.B)
        self.y = self.tan.load(w["src_q"])
        jv, _ = self.tan.tangent_batch(w["x0"])
        self.values0 = self.asm.precision_batch(w["q_values"], jv, self.noise)
        self.F.factor(self.asm.pattern, w["n_blocks"], values=self.values0)

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def run(self, gn, max_steps, rtol, device=True):
        w = self.w
        conv = self.dev if device else (lambda a: a)
        x, steps, hist = gn.run(conv(w["q_values"]), conv(w["Qx_prior"]), conv(w["x_prior"]), conv(w["x0"]), y=conv(self.y),
                                noise=self.noise, rtol=rtol, max_steps=max_steps)
        return (x.cpu().numpy() if device else x), steps, hist


def single_device_loop(pkg, w, p, n_steps):
    """The one-problem device loop (`gn_step` on a batch-1 handle with an order-2 tangent) for problem p: n_steps iterations, no
    stop rule.  Returns the list of iterates."""
    import torch
    tan = pkg.EllipticP1Tangent(w["nx"], w["ny"], order=2)
    asm = pkg.PosteriorAssembler(w["Q"], tan.pattern)
    qd, qx = torch.from_numpy(w["q_values"]).cuda(), torch.from_numpy(w["Qx_prior"][p]).cuda()
    b = tan.load(torch.from_numpy(w["src_q"][p]).cuda())
    x = torch.from_numpy(w["x0"][p].copy()).cuda()
    F, out = None, []
    for _ in range(n_steps):
        jv, fv = tan.tangent(x)
        if F is None:
            P = asm.pattern.copy(); P.data = asm.precision(qd, jv, w["noise"]).cpu().numpy()
            F = pkg.tridiagonal_cholesky(P, w["n_blocks"])
        x = pkg.gn_step(F, asm, qd, qx, jv, x, b - fv, w["noise"])
        out.append(x.cpu().numpy().copy())
    return out


def _route(pkg, gn):
    it, fw = C.c_int32(0), C.c_int32(0)
    pkg._cabi.check(pkg._cabi.load().gmrf_test_gn_route(gn._h, C.byref(it), C.byref(fw)))
    return it.value, fw.value


@pytest.mark.parametrize("nx,ny", MESHES)
def test_tangent_residual_and_load_against_the_oracle_entry_by_entry(pkg, nx, ny):
    """f_and_J (:280-285) and the load (:222) on the device against the cell-by-cell restatement, with the tolerances of the P1
    test: 1e-14 of max |J| for the values, 1e-13 of max(|.|, 1) for the vectors.  The restatement's own fp64-against-longdouble
    error on these meshes is at most 4.9e-16 max |J| and 9.9e-16 max(|f|, 1): a factor 20 and 100 below."""
    import torch
    mesh = PO.Mesh(nx, ny)
    rng = np.random.default_rng(8)
    X, Y = mesh.coords[:, 0], mesh.coords[:, 1]
    w = np.sin(np.pi * X) * np.sin(np.pi * Y) + 0.5 * np.cos(3 * X + Y) + 0.1 * rng.standard_normal(mesh.n)     # smooth + noise
    e = pkg.EllipticP1Tangent(nx, ny, order=2)
    d = pkg.DarcyP1Assembler(nx, ny, device=-1, order=2)
    assert e.qpoints.shape == (e.cells, 4, 2)
    src = np.cos(4 * e.qpoints[:, :, 0]) * (1.0 + e.qpoints[:, :, 1]) * 10.0 + rng.standard_normal(e.qpoints.shape[:2])
    sv, fs = PO.assemble_J_diff_and_f(mesh, src)
    fo, Jo = PO.f_and_J(w, mesh, sv, np.zeros(mesh.n))             # (the device residual carries no load)
    vals, f = e.tangent(w)
    b = e.load(src)
    for ref in (Jo, d.pattern):
        assert np.array_equal(e.pattern.indices, ref.indices) and np.array_equal(e.pattern.indptr, ref.indptr)
    ev, ef, eb = np.max(np.abs(vals - Jo.data)), np.max(np.abs(f - fo)), np.max(np.abs(b - fs))
    print(f"{nx}x{ny}: max |J| {np.max(np.abs(Jo.data)):.3e} err {ev:.2e}; max |f| {np.max(np.abs(fo)):.3e} err {ef:.2e}; "
          f"max |b| {np.max(np.abs(fs)):.3e} err {eb:.2e}")
    assert ev < 1e-14 * np.max(np.abs(Jo.data))
    assert ef < 1e-13 * max(np.max(np.abs(fo)), 1.0)
    assert eb < 1e-13 * max(np.max(np.abs(fs)), 1.0)
    # prescribed rows are exactly zero, interior ones are not
    J = sp.csr_matrix((vals, e.pattern.indices, e.pattern.indptr), shape=e.pattern.shape).toarray()
    pres = sorted(mesh.prescribed)
    interior = sorted(set(range(mesh.n)) - mesh.prescribed)
    assert len(interior) == (2 * nx - 3) * (2 * ny - 3)
    assert not np.any(J[pres]) and not np.any(f[pres]) and not np.any(b[pres])
    assert np.all(J[interior, interior] > 1.0) and np.all(b[interior] != 0.0) and np.all(f[interior] != 0.0)
    # device-resident operands: the same bits
    vd, fd = e.tangent(torch.from_numpy(w).cuda())
    bd = e.load(torch.from_numpy(src).cuda())
    assert vd.is_cuda and np.array_equal(vd.cpu().numpy(), vals) and np.array_equal(fd.cpu().numpy(), f)
    assert bd.is_cuda and np.array_equal(bd.cpu().numpy(), b)


@pytest.mark.parametrize("nx,ny", MESHES)
def test_batch_calls_are_bitwise_the_one_problem_calls(pkg, nx, ny):
    import torch
    B = 3
    e = pkg.EllipticP1Tangent(nx, ny, order=2)
    rng = np.random.default_rng(11)
    W = rng.standard_normal((B, e.n))
    S = rng.standard_normal((B, e.cells, 4))
    for device in (False, True):
        conv = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if device else (lambda a: a)
        back = (lambda t: t.cpu().numpy()) if device else (lambda a: a)
        vals, f = e.tangent_batch(conv(W))
        b = e.load(conv(S))
        assert (not device) or (vals.is_cuda and b.is_cuda)
        vals, f, b = back(vals), back(f), back(b)
        assert vals.shape == (B, e.nnz) and f.shape == (B, e.n) and b.shape == (B, e.n)
        for p in range(B):
            v1, f1 = e.tangent(conv(W[p]))
            b1 = e.load(conv(S[p]))
            assert np.array_equal(back(v1), vals[p]) and np.array_equal(back(f1), f[p]) and np.array_equal(back(b1), b[p])
        assert not np.array_equal(vals[0], vals[1]) and not np.array_equal(b[0], b[1])


@pytest.mark.parametrize("mesh_size", PO.GN_CASE_P2["meshes"])
def test_loop_against_the_oracle(pkg, gn_cases, mesh_size):
    """PO.GN_CASE_P2: the runs cut at 1, 2, 3 iterations to 1e-9 against the oracle's iterates; the full run's steps exactly, its
    final iterate and history to 2 x the one-problem device loop's error against the same oracle + 1e-12 (the rule of
    tests/test_gpu_elliptic.py::test_loop_against_the_oracle); a frozen problem's x bitwise unchanged by the later iterations; host
    and device inputs give the same bits; the driver ran max(steps) iterations."""
    c = PO.GN_CASE_P2
    w, prob, (xo, so, ho, rels, its) = gn_cases[mesh_size]
    s = Setup(pkg, w)
    assert s.tan.n == w["n"] and s.F.stats()["block_size"] == {(8, 8): 75, (10, 8): 95}[mesh_size]
    gn = pkg.GaussNewtonBatch(s.F, s.asm, s.tan)
    for k in (1, 2, 3):
        x, steps, hist = s.run(gn, k, c["rtol"])
        assert np.array_equal(steps, np.minimum(so, k))
        for p in range(c["B"]):
            e = rel(x[p], its[k - 1][p])
            print(f"max_steps={k} p={p} rel {e:.2e}")
            assert e < 1e-9
            assert np.all(np.isfinite(hist[p, :k + 1])) and np.all(np.isnan(hist[p, k + 1:]))
    x, steps, hist = s.run(gn, c["max_steps"], c["rtol"])
    assert _route(pkg, gn)[0] == int(so.max())
    xh, sh, hh = s.run(gn, c["max_steps"], c["rtol"], device=False)
    assert np.array_equal(xh, x) and np.array_equal(sh, steps) and np.array_equal(hh, hist, equal_nan=True)
    print("steps", steps, "oracle", so)
    assert np.array_equal(steps, so)
    assert len(set(steps.tolist())) >= 2
    for p in range(c["B"]):
        n_p = int(so[p])
        assert np.all(np.isnan(hist[p, n_p + 1:])) and np.all(np.isfinite(hist[p, :n_p + 1]))
        single = single_device_loop(pkg, w, p, n_p)
        fJ = prob.fJ(p)
        h_single = [ho[p, 0]]
        for xs in single:
            f, _ = fJ(xs)
            h_single.append(GO.objective(w["Q"], w["x_prior"][p], xs, -f, w["noise"]))
        e_b, e_s = rel(x[p], xo[p]), rel(single[-1], xo[p])
        eh_b, eh_s = rel(hist[p, :n_p + 1], ho[p, :n_p + 1]), rel(h_single, ho[p, :n_p + 1])
        err = pkg.workloads.solution_errors(x[p], w["truth"][p])
        print(f"p={p} steps={n_p}: x batch {e_b:.2e} single {e_s:.2e}; history batch {eh_b:.2e} single {eh_s:.2e}; vs truth {err}")
        assert e_b <= 2 * e_s + 1e-12
        assert eh_b <= 2 * eh_s + 1e-12
    # frozen: the problem that stops first -- in a run cut at its own count it has just arrived at the x it keeps to the end
    p0 = int(np.argmin(so))
    xc, sc, _ = s.run(gn, int(so[p0]), c["rtol"])
    assert sc[p0] == so[p0] and np.array_equal(xc[p0], x[p0])


def test_finalize_leaves_the_factor_at_the_final_iterate(pkg, gn_cases):
    """logdet and the posterior mean of the batch handle after finalize() against a one-problem handle factored from values
    assembled through the one-problem order-2 calls at the same x: 1e-10 of |logdet|; solve_tol (0.25 cond eps, two
    backward-stable factorisations of one matrix) for the mean."""
    c = PO.GN_CASE_P2
    w = gn_cases[(10, 8)][0]
    s = Setup(pkg, w)
    gn = pkg.GaussNewtonBatch(s.F, s.asm, s.tan)
    x, steps, _ = s.run(gn, c["max_steps"], c["rtol"])
    assert gn.finalize() is s.F
    tan1 = pkg.EllipticP1Tangent(w["nx"], w["ny"], order=2)
    asm1 = pkg.PosteriorAssembler(w["Q"], tan1.pattern)
    rhs, means, tols = np.empty_like(x), [], []
    for p in range(c["B"]):
        jv, _ = tan1.tangent(x[p])
        A = asm1.pattern.copy(); A.data = asm1.precision(w["q_values"], jv, w["noise"])
        F1 = pkg.tridiagonal_cholesky(A, w["n_blocks"])
        s.F.select_problem(p)
        ld, ld1 = s.F.logdet(), F1.logdet()
        print(f"p={p}: logdet batch {ld:.15e} one-problem {ld1:.15e}")
        assert abs(ld - ld1) <= 1e-10 * abs(ld1)
        rhs[p] = A @ x[p]
        means.append(pkg.ldiv(F1, rhs[p]))
        tols.append(solve_tol(types.SimpleNamespace(Q=A.tocsc(), meta={})))
    mean, smp = s.F.posterior_batch(s.dev(rhs), 16)
    mean = mean.cpu().numpy()
    for p in range(c["B"]):
        print(f"p={p}: mean vs one-problem handle {rel(mean[p], means[p]):.2e}, vs x {rel(mean[p], x[p]):.2e}, tol {tols[p]:.2e}")
        assert rel(mean[p], means[p]) < tols[p] and rel(mean[p], x[p]) < tols[p]
    assert smp.shape == (c["B"], 16, w["n"])


def test_a_problem_does_not_depend_on_its_batch(pkg, gn_cases):
    """The problem with amp 1 (index 2 of the case) alone in a batch-1 handle: the same bits as in the batch of 4."""
    c = PO.GN_CASE_P2
    w4, _, (_, so, _, _, _) = gn_cases[(10, 8)]
    p = c["amps"].index(1.0)
    w1 = pkg.workloads.elliptic_gauss_newton_batch((10, 8), 1, rows_per_block=c["rows_per_block"], amps=[1.0], order=2)
    assert np.array_equal(w1["src_q"][0], w4["src_q"][p])
    out = []
    for w in (w4, w1):
        s = Setup(pkg, w)
        gn = pkg.GaussNewtonBatch(s.F, s.asm, s.tan)
        out.append(s.run(gn, c["max_steps"], c["rtol"]))
    (x4, s4, h4), (x1, s1, h1) = out
    print(f"steps {s4[p]} / {s1[0]}, rel {rel(x1[0], x4[p]):.2e}")
    assert s4[p] == s1[0] == so[p]
    assert np.array_equal(x4[p], x1[0]) and np.array_equal(h4[p], h1[0], equal_nan=True)


def test_errors_and_the_p1_loop_beside_it(pkg, gn_cases):
    import torch
    cabi = pkg._cabi
    c = PO.GN_CASE_P2
    w = gn_cases[(8, 8)][0]

    def refused(fn, status=cabi.ERR_BAD_SHAPE):
        with pytest.raises(pkg.GmrfError) as e:
            fn()
        assert e.value.status == status

    # a P1 elliptic loop before the P2 one (EO.GN_CASE on 16 x 16, 3 iterations)
    def p1_run():
        c1 = EO.GN_CASE
        w1 = pkg.workloads.elliptic_gauss_newton_batch((16, 16), c1["B"], rows_per_block=c1["rows_per_block"], amps=c1["amps"])
        s1 = Setup(pkg, w1)
        assert s1.tan.order == 1 and s1.tan.nq == 3
        return s1.run(pkg.GaussNewtonBatch(s1.F, s1.asm, s1.tan), 3, c1["rtol"])

    before = p1_run()
    s = Setup(pkg, w)
    stream = s.stream.cuda_stream
    # the 15 x 15 lattice has the dofs of a 15 x 15 P1 mesh, on another pattern: an order-2 tangent with an assembler built on the
    # P1 pattern is refused, and so is a P1 tangent with the assembler of the lattice
    p1_tan = pkg.EllipticP1Tangent(15, 15, stream=stream)
    assert p1_tan.n == s.tan.n == 225 and p1_tan.nnz != s.tan.nnz
    p1_asm = pkg.PosteriorAssembler(w["Q"], p1_tan.pattern, stream=stream)
    refused(lambda: pkg.GaussNewtonBatch(s.F, p1_asm, s.tan))
    refused(lambda: pkg.GaussNewtonBatch(s.F, s.asm, p1_tan))
    refused(lambda: pkg.GaussNewtonBatch(s.F, s.asm, pkg.EllipticP1Tangent(w["nx"], w["ny"], device=-1, order=2)))
    with pytest.raises(ValueError):                                 # the P1 rule's three points per cell
        s.tan.load(np.zeros((s.tan.cells, 3)))
    with pytest.raises(ValueError):
        s.tan.load(np.zeros((2, s.tan.cells, 3)))
    gn = pkg.GaussNewtonBatch(s.F, s.asm, s.tan)
    good = s.run(gn, 3, c["rtol"])
    assert good[1].tolist() == [3, 3, 3, 3]
    # the P1 loop after the P2 one: the same bits
    after = p1_run()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2], equal_nan=True)
    assert before[1].tolist() == [3, 3, 3, 3]
    torch.cuda.synchronize()
