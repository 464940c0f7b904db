"""Batched device-resident Gauss-Newton (gmrf_gn_run) for the Burgers data-set loop against tests/gn_batch_oracle.py and
against the one-problem device loop (`gn_step`)."""
import ctypes as C
import types

import numpy as np
import pytest

import __graft_entry__
from oracle import bt_oracle as O
from tests import gn_batch_oracle as GO
from tests.test_gpu_parity import rel, solve_tol

pytestmark = pytest.mark.gpu

Switch = __graft_entry__.load_package().Switch


class Setup:
    """Handle, assembler and tangent on ONE stream, the handle factored once on the assembler's pattern (values at x0)."""

    def __init__(self, pkg, ns, nt, B, seed=0, order=1, w=None, analyse=True, handle_order="reference"):
        import torch
        self.torch = torch
        self.w = w if w is not None else pkg.workloads.burgers_gauss_newton_batch(ns, nt, B, seed=seed)
        w = self.w
        self.ns, self.nt, self.B, self.noise = ns, nt, B, w["noise"]
        self.stream = torch.cuda.Stream()
        s = self.stream.cuda_stream
        self.tan = pkg.BurgersP1Tangent(ns, nt, w["dt"], w["nu"], stream=s, order=order)
        self.asm = pkg.PosteriorAssembler(w["Q"], self.tan.pattern, stream=s)
        self.F = pkg.TridiagonalCholeskyFactor(stream=s, batch=B, order=handle_order)
        if analyse:
            self.values0 = self.first_values()
            self.F.factor(self.asm.pattern, nt, values=self.values0)

    def first_values(self):
        jv, _ = self.tan.tangent_batch(self.w["x0"])
        return self.asm.precision_batch(self.w["q_values"], jv, self.noise)

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def run(self, gn, max_steps, rtol, device=True, q_values=None, **kw):
        w = self.w
        conv = self.dev if device else (lambda a: a)
        q = w["q_values"] if q_values is None else q_values
        x, steps, hist = gn.run(conv(q), conv(w["Qx_prior"]), conv(w["x_prior"]), conv(w["x0"]), noise=self.noise, rtol=rtol,
                                max_steps=max_steps, **kw)
        return (x.cpu().numpy() if device else x), steps, hist


def single_device_loop(pkg, w, p, n_steps, ns, nt):
    """The existing one-problem device loop (`gn_step` on a batch-1 handle) for problem p: n_steps iterations, no stop rule.
    Returns the list of iterates."""
    import torch
    b = pkg.BurgersP1Tangent(ns, nt, w["dt"], w["nu"])
    Q = GO.problem_matrix(w["Q"], w["q_values"][p])
    asm = pkg.PosteriorAssembler(Q, b.pattern)
    qd, qx = torch.from_numpy(Q.data).cuda(), torch.from_numpy(w["Qx_prior"][p]).cuda()
    x = torch.from_numpy(w["x0"][p].copy()).cuda()
    F, out = None, []
    for _ in range(n_steps):
        jv, fv = b.tangent(x)
        if F is None:
            P = asm.pattern.copy(); P.data = asm.precision(qd, jv, w["noise"]).cpu().numpy()
            F = pkg.tridiagonal_cholesky(P, nt)
        x = pkg.gn_step(F, asm, qd, qx, jv, x, -fv, w["noise"])
        out.append(x.cpu().numpy().copy())
    return out


def oracle_case(pkg, c):
    w = pkg.workloads.burgers_gauss_newton_batch(c["ns"], c["nt"], c["B"], seed=c["seed"])
    res = GO.batch_loop(c["ns"], c["nt"], w["dt"], w["nu"], w["Q"], w["q_values"], w["Qx_prior"], w["x_prior"], w["x0"], w["noise"],
                        c["nt"], c["rtol"], c["max_steps"])
    return w, res


@pytest.mark.parametrize("order", [1, 2])
def test_building_blocks_are_bitwise_the_one_problem_calls(pkg, order):
    import torch
    ns, nt, B = 64, 8, 5
    s = Setup(pkg, ns, nt, B, seed=5, order=order, analyse=False)
    w, tan, asm = s.w, s.tan, s.asm
    rng = np.random.default_rng(11)
    W = w["x0"] + 0.1 * rng.standard_normal(w["x0"].shape)
    od = rng.standard_normal((B, asm.m))
    for device in (False, True):
        conv = s.dev if device else (lambda a: a)
        back = (lambda t: t.cpu().numpy()) if device else (lambda a: a)
        vals, f = tan.tangent_batch(conv(W))
        assert (not device) or vals.is_cuda
        vals, f = back(vals), back(f)
        for qv, per_problem in ((w["q_values"], True), (w["q_values"][0], False)):
            A = back(asm.precision_batch(conv(qv), conv(vals), s.noise))
            r = back(asm.rhs_batch(conv(w["Qx_prior"]), conv(vals), conv(W), conv(od), s.noise))
            r0 = back(asm.rhs_batch(None, conv(vals), conv(W), None, s.noise))
            for p in range(B):
                v1, f1 = tan.tangent(conv(W[p]))
                assert np.array_equal(back(v1), vals[p]) and np.array_equal(back(f1), f[p])
                q1 = qv[p] if per_problem else qv
                assert np.array_equal(back(asm.precision(conv(q1), conv(vals[p]), s.noise)), A[p])
                assert np.array_equal(back(asm.rhs(conv(w["Qx_prior"][p]), conv(vals[p]), conv(W[p]), conv(od[p]), s.noise)), r[p])
                assert np.array_equal(back(asm.rhs(None, conv(vals[p]), conv(W[p]), None, s.noise)), r0[p])
    # the objective: the same bits for B = 1 and B = 5, across calls, host and device; NumPy's value to 1e-13
    for qv, per_problem in ((w["q_values"], True), (w["q_values"][0], False)):
        o5 = asm.objective_batch(qv, w["x_prior"], W, od, s.noise)
        assert np.array_equal(o5, asm.objective_batch(qv, w["x_prior"], W, od, s.noise))
        od5 = asm.objective_batch(s.dev(qv), s.dev(w["x_prior"]), s.dev(W), s.dev(od), s.noise)
        assert od5.is_cuda and np.array_equal(od5.cpu().numpy(), o5)
        for p in range(B):
            q1 = qv[p:p + 1] if per_problem else qv
            o1 = asm.objective_batch(q1, w["x_prior"][p:p + 1], W[p:p + 1], od[p:p + 1], s.noise)
            assert np.array_equal(o1, o5[p:p + 1])
            ref = GO.objective(GO.problem_matrix(w["Q"], qv[p] if per_problem else qv), w["x_prior"][p], W[p], od[p], s.noise)
            print(f"objective p={p}: device {o5[p]:.17e} numpy {ref:.17e} rel {abs(o5[p] - ref) / abs(ref):.2e}")
            assert abs(o5[p] - ref) <= 1e-13 * abs(ref)
    torch.cuda.synchronize()


def test_loop_against_the_oracle_64x8(pkg):
    """GO.GN_CASE (rtol 1e-5, see there): the first three iterations to 1e-9 as the one-problem loop is held; the full run's
    steps exactly, its final iterate and history to 2 x the one-problem device loop's error against the same oracle + 1e-12;
    a frozen problem's x bitwise unchanged by the later iterations."""
    c = GO.GN_CASE
    w, (xo, so, ho, rels, its) = oracle_case(pkg, c)
    s = Setup(pkg, c["ns"], c["nt"], c["B"], w=w)
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
    xh, sh, hh = s.run(gn, c["max_steps"], c["rtol"], device=False)
    assert np.array_equal(xh, x) and np.array_equal(sh, steps) and np.array_equal(hh, hist, equal_nan=True)
    print("steps", steps, "oracle", so)
    assert np.array_equal(steps, so)
    assert len(set(steps.tolist())) >= 2
    for p in range(c["B"]):
        n_p = int(so[p])
        assert np.all(np.isnan(hist[p, n_p + 1:])) and np.all(np.isfinite(hist[p, :n_p + 1]))
        single = single_device_loop(pkg, w, p, n_p, c["ns"], c["nt"])
        Q = GO.problem_matrix(w["Q"], w["q_values"][p])
        h_single = [ho[p, 0]]
        for xs in single:
            f, _ = O.burgers_f_and_J(c["ns"], c["nt"], w["dt"], w["nu"], xs)
            h_single.append(GO.objective(Q, w["x_prior"][p], xs, -f, w["noise"]))
        e_b, e_s = rel(x[p], xo[p]), rel(single[-1], xo[p])
        eh_b, eh_s = rel(hist[p, :n_p + 1], ho[p, :n_p + 1]), rel(h_single, ho[p, :n_p + 1])
        print(f"p={p} steps={n_p}: x batch {e_b:.2e} single {e_s:.2e}; history batch {eh_b:.2e} single {eh_s:.2e}")
        assert e_b <= 2 * e_s + 1e-12
        assert eh_b <= 2 * eh_s + 1e-12
    # frozen: the problem that stops first -- in a run cut at its own count it has just arrived at the x it keeps to the end
    p0 = int(np.argmin(so))
    xc, sc, _ = s.run(gn, int(so[p0]), c["rtol"])
    assert sc[p0] == so[p0] and np.array_equal(xc[p0], x[p0])


def test_a_problem_does_not_depend_on_its_batch(pkg):
    c = GO.GN_CASE
    ns, nt, B = c["ns"], c["nt"], c["B"]
    wa = pkg.workloads.burgers_gauss_newton_batch(ns, nt, B, seed=0)
    wb = pkg.workloads.burgers_gauss_newton_batch(ns, nt, B, seed=7)
    src, dst = 1, 4                      # problem 1 of batch a sits at index 4 of batch b, among other neighbours
    for k in ("q_values", "Qx_prior", "x_prior", "x0"):
        wb[k][dst] = wa[k][src]
    out = []
    for w in (wa, wb):
        s = Setup(pkg, ns, nt, B, w=w)
        gn = pkg.GaussNewtonBatch(s.F, s.asm, s.tan)
        out.append(s.run(gn, 4, c["rtol"]))
    (xa, sa, ha), (xb, sb, hb) = out
    assert sa[src] == sb[dst] == 4
    assert np.array_equal(xa[src], xb[dst]) and np.array_equal(ha[src], hb[dst])
    assert not np.array_equal(xa[dst], xb[dst])


def test_full_size_burgers512x64_against_oracle_and_one_problem_loop(pkg):
    """B = 8, 4 iterations; the oracle (seconds per step on the CPU) follows problems 0 and 5.  Measured on an MI355X:
    see DESIGN (section on the batched Gauss-Newton loop)."""
    ns, nt, B, k, rtol = 512, 64, 8, 4, 1e-4
    w = pkg.workloads.burgers_gauss_newton_batch(ns, nt, B, seed=0)
    s = Setup(pkg, ns, nt, B, w=w)
    gn = pkg.GaussNewtonBatch(s.F, s.asm, s.tan)
    x, steps, hist = s.run(gn, k, rtol)
    for p in (0, 5):
        Q = GO.problem_matrix(w["Q"], w["q_values"][p])
        xo, so, ho, iters = GO.single_loop(ns, nt, w["dt"], w["nu"], Q, w["Qx_prior"][p], w["x_prior"][p], w["x0"][p], w["noise"], nt,
                                           rtol, k)
        ratios = np.array([GO.rel_diff(ho[i], ho[i + 1]) for i in range(so)])
        assert GO.stop_margin(ratios, rtol) > 2.0          # (the stop decisions of this problem are not close calls)
        assert steps[p] == so
        single = single_device_loop(pkg, w, p, so, ns, nt)
        e_b, e_s = rel(x[p], xo), rel(single[-1], xo)
        print(f"burgers512x64 p={p} steps={so}: batched vs oracle {e_b:.3e}, one-problem gn_step loop vs oracle {e_s:.3e}")
        print(f"    objective history vs oracle {rel(hist[p, :so + 1], ho):.3e}")
        assert e_b <= 2 * e_s + 1e-12


def test_finalize_leaves_the_factor_at_the_final_iterate(pkg):
    c = GO.GN_CASE
    s = Setup(pkg, c["ns"], c["nt"], c["B"], seed=c["seed"])
    w = s.w
    gn = pkg.GaussNewtonBatch(s.F, s.asm, s.tan)
    x, steps, _ = s.run(gn, c["max_steps"], c["rtol"])
    assert gn.finalize() is s.F
    rhs, tols = np.empty_like(x), []
    for p in range(c["B"]):
        _, J = O.burgers_f_and_J(c["ns"], c["nt"], w["dt"], w["nu"], x[p])
        A = O.assemble_posterior(GO.problem_matrix(w["Q"], w["q_values"][p]), J, w["noise"])
        s.F.select_problem(p)
        ld, ld_o = s.F.logdet(), O.logdet(O.tridiagonal_cholesky(A, c["nt"]))
        assert abs(ld - ld_o) <= 1e-10 * abs(ld_o)
        rhs[p] = A @ x[p]
        tols.append(solve_tol(types.SimpleNamespace(Q=A, meta={})))
    mean, smp = s.F.posterior_batch(s.dev(rhs), 16)
    mean = mean.cpu().numpy()
    for p in range(c["B"]):
        assert rel(mean[p], x[p]) < tols[p]
    assert smp.shape == (c["B"], 16, c["ns"] * c["nt"])


def _route(pkg, gn):
    it, fw = C.c_int32(0), C.c_int32(0)
    pkg._cabi.check(pkg._cabi.load().gmrf_test_gn_route(gn._h, C.byref(it), C.byref(fw)))
    return it.value, fw.value


@pytest.mark.parametrize("ns,nt,B,expected", [(64, 8, 6, False), (512, 64, 16, True)])
def test_forward_in_factor_route(pkg, lib, ns, nt, B, expected):
    """One iteration with and without set_eager bit 19.  Whether the route qualifies for this block size is asked of the handle
    itself (a registered right-hand side, a re-factorisation, gmrf_test_factor_fwd); where it does the run must have taken it
    and the two results agree to 1e-12, where it does not they are bitwise equal.  Blocks of 64 never qualify (no 256-column
    panels); burgers512x64 does as a batch of 16, the case tests/test_gpu_factor_forward.py runs (a batch of 8 has too few
    tiles for the products that carry the tail row)."""
    s = Setup(pkg, ns, nt, B)
    probe = s.dev(s.w["Qx_prior"])
    s.F.set_factor_rhs(probe)
    s.F.refactor(s.values0)
    state = C.c_int32(0)
    pkg._cabi.check(lib.gmrf_test_factor_fwd(s.F._h, C.byref(state), None))
    qualifies = state.value == 1
    s.F.set_factor_rhs(None)
    gn = pkg.GaussNewtonBatch(s.F, s.asm, s.tan)
    x_on, _, h_on = s.run(gn, 1, 1e-4)
    assert _route(pkg, gn) == (1, 1 if qualifies else 0)
    pkg._cabi.check(lib.gmrf_test_factor_fwd(s.F._h, C.byref(state), None))
    assert state.value == 0                               # (the run's registration does not outlive it)
    s.F.set_eager(Switch.NO_FACTOR_FWD)
    x_off, _, h_off = s.run(gn, 1, 1e-4)
    assert _route(pkg, gn) == (1, 0)
    s.F.set_eager(0)
    print(f"{ns}x{nt}: route qualifies {qualifies}, rel {max(rel(x_on[p], x_off[p]) for p in range(B)):.2e}")
    if qualifies:
        assert all(rel(x_on[p], x_off[p]) < 1e-12 for p in range(B))
    else:
        assert np.array_equal(x_on, x_off) and np.array_equal(h_on, h_off)
    assert qualifies == expected


def test_errors_and_the_one_problem_handle(pkg):
    import torch
    cabi = pkg._cabi
    c = GO.GN_CASE
    ns, nt, B = c["ns"], c["nt"], c["B"]
    s = Setup(pkg, ns, nt, B, seed=c["seed"])
    w = s.w

    def refused(fn, status=cabi.ERR_BAD_SHAPE):
        with pytest.raises(pkg.GmrfError) as e:
            fn()
        assert e.value.status == status

    # another stream, a pattern-only part, another mesh: refused when bound
    other = pkg.BurgersP1Tangent(ns, nt, w["dt"], w["nu"])
    refused(lambda: pkg.GaussNewtonBatch(s.F, s.asm, other))
    refused(lambda: pkg.GaussNewtonBatch(s.F, pkg.PosteriorAssembler(w["Q"], s.tan.pattern, device=-1), s.tan))
    refused(lambda: pkg.GaussNewtonBatch(s.F, s.asm, pkg.BurgersP1Tangent(ns, nt + 1, w["dt"], w["nu"], stream=s.stream.cuda_stream)))
    # a twisted handle
    tw = Setup(pkg, ns, nt, 1, analyse=False, handle_order="twisted")
    refused(lambda: pkg.GaussNewtonBatch(tw.F, tw.asm, tw.tan))
    # before the first analysis; a handle that analysed another pattern; a batch that is not the handle's
    fresh = Setup(pkg, ns, nt, B, w=w, analyse=False)
    gn_fresh = pkg.GaussNewtonBatch(fresh.F, fresh.asm, fresh.tan)
    refused(lambda: fresh.run(gn_fresh, 2, 1e-4), cabi.ERR_NO_FACTOR)
    fresh.F.factor(w["Q"], nt, values=w["q_values"])             # (Q's own pattern, not the assembler's)
    if w["Q"].nnz != fresh.asm.nnz_out:
        refused(lambda: fresh.run(gn_fresh, 2, 1e-4))
    gn = pkg.GaussNewtonBatch(s.F, s.asm, s.tan)
    refused(lambda: gn.run(w["q_values"][:B - 1], w["Qx_prior"][:B - 1], w["x_prior"][:B - 1], w["x0"][:B - 1], noise=s.noise))
    with pytest.raises(ValueError):
        gn.run(w["q_values"], w["Qx_prior"][:, :-1], w["x_prior"], w["x0"], noise=s.noise)
    # one problem made indefinite: NotPositiveDefinite with the block; x holds the last complete iterates; the handle goes on
    good = s.run(gn, 3, c["rtol"])
    bad_q = w["q_values"].copy()
    Q = w["Q"]
    blk = 5
    j = (blk - 1) * ns + 3                                        # a diagonal entry of block 5 (1-based) of problem 2
    e = Q.indptr[j] + int(np.searchsorted(Q.indices[Q.indptr[j]:Q.indptr[j + 1]], j))
    assert Q.indices[e] == j
    bad_q[2, e] = -1e30
    with pytest.raises(pkg.NotPositiveDefinite) as ei:
        s.run(gn, 3, c["rtol"], q_values=bad_q)
    assert ei.value.info == blk
    x_last, steps_last, _ = gn.last
    assert np.array_equal(steps_last, np.zeros(B, dtype=np.int32)) and np.array_equal(x_last.cpu().numpy(), w["x0"])
    again = s.run(gn, 3, c["rtol"])
    assert np.array_equal(again[0], good[0]) and np.array_equal(again[1], good[1])
    # a reference-order handle with batch 1: the one-problem gn_step loop's iterates
    p = 3
    w1 = {k: (v[p:p + 1] if isinstance(v, np.ndarray) and v.ndim == 2 and k != "ic" else v) for k, v in w.items()}
    s1 = Setup(pkg, ns, nt, 1, w=w1)
    gn1 = pkg.GaussNewtonBatch(s1.F, s1.asm, s1.tan)
    single = single_device_loop(pkg, w, p, 3, ns, nt)
    for k in (1, 2, 3):
        x1, st1, _ = s1.run(gn1, k, c["rtol"])
        assert st1[0] == k and rel(x1[0], single[k - 1]) < 1e-9
    torch.cuda.synchronize()


def test_neighbouring_calls_are_unchanged_by_a_run(pkg):
    c = GO.GN_CASE
    s = Setup(pkg, c["ns"], c["nt"], c["B"], seed=c["seed"])
    b = s.dev(s.w["Qx_prior"])
    before = s.F.solve_batch(b[:, None, :]).cpu().numpy()
    m0, smp0 = s.F.posterior_batch(b, 16)
    gn = pkg.GaussNewtonBatch(s.F, s.asm, s.tan)
    s.run(gn, 3, c["rtol"])
    s.F.refactor(s.values0)
    assert np.array_equal(s.F.solve_batch(b[:, None, :]).cpu().numpy(), before)
    m1, smp1 = s.F.posterior_batch(b, 16)
    assert np.array_equal(m1.cpu().numpy(), m0.cpu().numpy()) and np.array_equal(smp1.cpu().numpy(), smp0.cpu().numpy())
