"""The Burgers line tangent over (order, scheme, bc) on the device (gmrf_burgers_line_create behind the gmrf_burgers_p1_* calls)
against tests/burgers_cn_oracle.py, and the batched Gauss-Newton loop bound to the Crank-Nicolson / Dirichlet tangent on the
benchmark of workloads.burgers_chen24_batch, by the rules of tests/test_gpu_elliptic_p2.py."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import burgers_cn_oracle as BO
from tests.test_gpu_parity import rel

pytestmark = pytest.mark.gpu

COMBOS = list(itertools.product((1, 2), ("euler", "cn"), ("periodic", "dirichlet")))
DT, NU, LENGTH = 0.05, 0.01, 2.0


def shapes(bc):
    """The smallest mesh of the bc on 2 slices; 5 cells x 4 slices; 67 cells x 5 slices: 268 to 540 rows, which crosses a
    256-row workgroup boundary and leaves a ragged last workgroup for every (order, bc)."""
    return ((3 if bc == "periodic" else 2, 2), (5, 4), (67, 5))


def dofs(nc, order, bc):
    return order * nc + (1 if bc == "dirichlet" else 0)


def smooth_plus_noise(ns, nt, seed):
    x, t = np.arange(ns) / ns, np.arange(nt)[:, None]
    return (np.sin(2 * np.pi * x)[None, :] * (1.0 - 0.1 * t) + 0.3 * np.cos(6 * np.pi * x + t) +
            0.1 * np.random.default_rng(seed).standard_normal((nt, ns))).ravel()


def tangent(pkg, nc, nt, order, scheme, bc, length=LENGTH):
    """(On a line of length 2 every combination, euler / periodic too, runs the kernels of burgers_line.hpp.)"""
    return pkg.BurgersP1Tangent(dofs(nc, order, bc), nt, DT, NU, order=order, scheme=scheme, bc=bc, length=length)


def blocks(b, vals):
    """Dense J as [row slice - 1, i, column slice, j]."""
    import scipy.sparse as sp
    J = sp.csr_matrix((vals, b.pattern.indices, b.pattern.indptr), shape=b.pattern.shape)
    return J.toarray().reshape(b.nt - 1, b.ns, b.nt, b.ns)


@pytest.fixture(scope="module")
def chen(pkg):
    """BO.CHEN_CASE under both schemes, computed once and left unchanged: scheme -> (workload, fJ, batch_loop result)."""
    return {s: BO.chen_case(pkg.workloads, s) for s in ("cn", "euler")}


@pytest.mark.parametrize("order,scheme,bc", COMBOS)
def test_tangent_against_the_oracle_entry_by_entry(pkg, order, scheme, bc):
    """Values to 1e-14 of max |J|, f to 1e-13 of max(|f|, 1): the bounds of tests/test_gpu_elliptic_p2.py:106-108.  On the
    Dirichlet interval the stored values in the rows and columns of dofs 0 and ns-1, and f at those rows, are exactly 0.0."""
    for nc, nt in shapes(bc):
        b = tangent(pkg, nc, nt, order, scheme, bc)
        w = smooth_plus_noise(b.ns, nt, 8)
        fo, Jo = BO.f_and_J(nc, nt, DT, NU, w, order, scheme, bc, LENGTH)
        vals, f = b.tangent(w)
        assert np.array_equal(b.pattern.indices, Jo.indices) and np.array_equal(b.pattern.indptr, Jo.indptr)
        ev, ef = np.max(np.abs(vals - Jo.data)), np.max(np.abs(f - fo))
        print(f"order {order} {scheme} {bc} {nc}x{nt}: max |J| {np.max(np.abs(Jo.data)):.3e} err {ev:.2e}; max |f| {np.max(np.abs(fo)):.3e} err {ef:.2e}")
        assert ev <= 1e-14 * np.max(np.abs(Jo.data))
        assert ef <= 1e-13 * max(np.max(np.abs(fo)), 1.0)
        if bc == "dirichlet":
            ends = [0, b.ns - 1]
            row_dof = np.repeat(np.arange(b.rows), np.diff(b.pattern.indptr)) % b.ns
            touched = np.isin(row_dof, ends) | np.isin(b.pattern.indices % b.ns, ends)
            assert touched.sum() > 0 and np.all(vals[touched] == 0.0) and np.all(f.reshape(nt - 1, b.ns)[:, ends] == 0.0)
            assert np.all(vals[~touched] != 0.0) and np.all(f.reshape(nt - 1, b.ns)[:, 1:-1] != 0.0)


@pytest.mark.parametrize("order,bc", list(itertools.product((1, 2), ("periodic", "dirichlet"))))
def test_crank_nicolson_against_the_euler_kernel(pkg, order, bc):
    """Independent of the oracle: with M read off the Euler tangent (-J_euler[block t, t-1]) on the same mesh and w,
        J_cn[:, t] = (J_euler[:, t] + M) / 2   and, for t >= 2,   J_cn[block t, t-1] = J_euler[block t-1, t-1] / 2 - 3/2 M.
    Each device value is within 1e-14 max |J| of the exact one (the parity bound above), so the two sides differ by at most
    (1 + 1/2 + 1/2) and (1 + 1/2 + 3/2) times that."""
    nc, nt = 67, 5
    length = 1.0 if bc == "periodic" else LENGTH        # (periodic, length 1: the Euler side is burgers_p1_rows_batch / burgers_p2_rows_batch)
    be, bc_ = tangent(pkg, nc, nt, order, "euler", bc, length), tangent(pkg, nc, nt, order, "cn", bc, length)
    w = smooth_plus_noise(be.ns, nt, 9)
    ve, _ = be.tangent(w)
    vc, _ = bc_.tangent(w)
    Je, Jc = blocks(be, ve), blocks(bc_, vc)
    M = -Je[0, :, 0, :]
    scale = 1e-14 * max(np.max(np.abs(ve)), np.max(np.abs(vc)))
    for t in range(1, nt):
        e1 = np.max(np.abs(Jc[t - 1, :, t, :] - 0.5 * (Je[t - 1, :, t, :] + M)))
        assert e1 <= 2 * scale, (t, e1, scale)
        if t >= 2:
            e2 = np.max(np.abs(Jc[t - 1, :, t - 1, :] - (0.5 * Je[t - 2, :, t - 1, :] - 1.5 * M)))
            assert e2 <= 3 * scale, (t, e2, scale)
    assert np.max(np.abs(Jc[0, :, 0, :] + M)) > 100 * scale          # (the t-1 block is not Euler's -M)


@pytest.mark.parametrize("order,scheme,bc", COMBOS)
def test_bits(pkg, order, scheme, bc):
    """The batch call is the one-problem call bit for bit, device tensors give the bits of host arrays, two problems of a batch
    differ; euler / periodic through the new constructor gives the bits of gmrf_burgers_p1_create / _p2_create."""
    import torch
    nc, nt, B = 67, 5, 3
    b = tangent(pkg, nc, nt, order, scheme, bc, length=1.0 if (scheme, bc) == ("euler", "periodic") else LENGTH)
    W = np.stack([smooth_plus_noise(b.ns, nt, 20 + p) for p in range(B)])
    vals, f = b.tangent_batch(W)
    vd, fd = b.tangent_batch(torch.from_numpy(W).cuda())
    assert vd.is_cuda and np.array_equal(vd.cpu().numpy(), vals) and np.array_equal(fd.cpu().numpy(), f)
    assert vals.shape == (B, b.nnz) and f.shape == (B, b.rows)
    for p in range(B):
        v1, f1 = b.tangent(W[p])
        v1d, f1d = b.tangent(torch.from_numpy(W[p]).cuda())
        assert np.array_equal(v1, vals[p]) and np.array_equal(f1, f[p])
        assert np.array_equal(v1d.cpu().numpy(), vals[p]) and np.array_equal(f1d.cpu().numpy(), f[p])
    assert not np.array_equal(vals[0], vals[1]) and not np.array_equal(f[0], f[1])
    if (scheme, bc) == ("euler", "periodic"):
        lib, cabi = pkg._cabi.load(), pkg._cabi
        h = C.c_void_p()
        cabi.check((lib.gmrf_burgers_p2_create if order == 2 else lib.gmrf_burgers_p1_create)(0, None, b.ns, nt, DT, NU, C.byref(h)))
        vo, fo = np.empty(b.nnz), np.empty(b.rows)
        cabi.check(lib.gmrf_burgers_p1_tangent(h, cabi.ptr(W[0]), cabi.ptr(vo), cabi.ptr(fo)))
        vb, fb = np.empty((B, b.nnz)), np.empty((B, b.rows))
        cabi.check(lib.gmrf_burgers_p1_tangent_batch(h, B, cabi.ptr(W), cabi.ptr(vb), cabi.ptr(fb)))
        lib.gmrf_burgers_p1_destroy(h)
        assert np.array_equal(vo, vals[0]) and np.array_equal(fo, f[0]) and np.array_equal(vb, vals) and np.array_equal(fb, f)


class Setup:
    """Handle, assembler and tangent on ONE stream, the handle factored once on the assembler's pattern (values at x0)."""

    def __init__(self, pkg, w, scheme):
        import torch
        self.torch, self.w = torch, w
        self.B, self.noise = w["x0"].shape[0], w["noise"]
        self.stream = torch.cuda.Stream()
        s = self.stream.cuda_stream
        self.tan = pkg.BurgersP1Tangent(w["ns"], w["n_blocks"], w["dt"], w["nu"], stream=s, order=w["order"], scheme=scheme,
                                        bc="dirichlet", length=w["length"])
        self.asm = pkg.PosteriorAssembler(w["Q"], self.tan.pattern, stream=s)
        self.F = pkg.TridiagonalCholeskyFactor(stream=s, batch=self.B)
        jv, _ = self.tan.tangent_batch(w["x0"])
        self.F.factor(self.asm.pattern, w["n_blocks"], values=self.asm.precision_batch(w["q_values"], jv, self.noise))

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def run(self, gn, max_steps, rtol):
        w = self.w
        x, steps, hist = gn.run(self.dev(w["q_values"]), self.dev(w["Qx_prior"]), self.dev(w["x_prior"]), self.dev(w["x0"]),
                                noise=self.noise, rtol=rtol, max_steps=max_steps)
        return x, steps, hist


def device_rel_err(pkg, w, x):
    """rel_err of the last slice against Cole-Hopf on the device (solution_errors_batch over [(nt-1) ns, n))."""
    import torch
    soln = np.zeros((x.shape[0], w["n"]))
    soln[:, -w["ns"]:] = w["truth"]
    return pkg.solution_errors_batch(x, torch.from_numpy(soln).cuda(), first=(w["n_blocks"] - 1) * w["ns"])[:, 0]


def test_loop_against_the_oracle(pkg, chen):
    """BO.CHEN_CASE, n = 1690 in 26 blocks of 65: the runs cut at 1, 2, 3 iterations to 1e-9 against the oracle's iterates; the
    full run's steps exactly the oracle's, with at least two different counts in the batch; rel_err against Cole-Hopf at T = 1
    within 1 % of the oracle's own; Crank-Nicolson below 0.2 x implicit Euler on the device as on the oracle."""
    c = BO.CHEN_CASE
    errs = {}
    for scheme in ("cn", "euler"):
        w, _, (xo, so, ho, _, its) = chen[scheme]
        s = Setup(pkg, w, scheme)
        assert s.tan.n == w["n"] == 1690 and s.F.stats()["block_size"] == 65
        gn = pkg.GaussNewtonBatch(s.F, s.asm, s.tan)
        if scheme == "cn":
            for k in (1, 2, 3):
                x, steps, hist = s.run(gn, k, c["rtol"])
                assert np.array_equal(steps, np.minimum(so, k))
                for p in range(c["B"]):
                    e = rel(x[p].cpu().numpy(), its[k - 1][p])
                    print(f"max_steps={k} p={p} rel {e:.2e}")
                    assert e < 1e-9
                    assert np.all(np.isfinite(hist[p, :k + 1])) and np.all(np.isnan(hist[p, k + 1:]))
        x, steps, hist = s.run(gn, c["max_steps"], c["rtol"])
        print(scheme, "steps", steps, "oracle", so)
        assert np.array_equal(steps, so)
        assert len(set(steps.tolist())) >= 2
        errs[scheme] = device_rel_err(pkg, w, x)
        eo = BO.last_slice_rel_err(w, xo)
        print(scheme, "rel_err device", errs[scheme], "oracle", eo, "x vs oracle", [rel(x[p].cpu().numpy(), xo[p]) for p in range(c["B"])])
        assert np.all(np.abs(errs[scheme] - eo) <= 0.01 * eo)
    assert np.all(errs["cn"] < 0.2 * errs["euler"])


def test_finalize_leaves_the_factor_at_the_final_iterate(pkg, chen):
    """logdet of every problem against the oracle's factor (SuperLU) of Q + noise J'J at the device's final iterate to 1e-10
    relative; the exact marginal variances finite and positive."""
    c = BO.CHEN_CASE
    w, fJ, _ = chen["cn"]
    s = Setup(pkg, w, "cn")
    gn = pkg.GaussNewtonBatch(s.F, s.asm, s.tan)
    x, steps, _ = s.run(gn, c["max_steps"], c["rtol"])
    assert gn.finalize() is s.F
    x = x.cpu().numpy()
    for p in range(c["B"]):
        s.F.select_problem(p)
        ld, ldo = s.F.logdet(), BO.logdet(BO.posterior_matrix(w["Q"], fJ(x[p])[1], w["noise"]))
        print(f"p={p}: logdet device {ld:.15e} oracle {ldo:.15e}")
        assert abs(ld - ldo) <= 1e-10 * abs(ldo)
    var = s.F.marginal_var("exact")
    assert var.shape == (c["B"], w["n"]) and np.all(np.isfinite(var)) and np.all(var > 0.0)
