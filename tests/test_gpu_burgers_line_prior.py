"""The batched device prior on every Burgers line (gmrf_burgers_line_prior_create behind the gmrf_burgers_prior_* calls) and the
initial-condition stage bound to it (gmrf_bic_*) against `workloads.burgers_line_prior_from_bulk`, the P1 stencil prior, SciPy and
tests/burgers_cn_oracle.py.  Shapes and bounds: tests/burgers_line_prior_checks.py."""
import ctypes as C
import types

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests import burgers_cn_oracle as BO
from tests import burgers_line_prior_checks as LP
from tests import burgers_prior_checks as BP
from tests import gn_batch_oracle as GO
from tests.test_gpu_burgers_prior import _check_ic_stage
from tests.test_gpu_parity import rel, solve_tol

pytestmark = pytest.mark.gpu

FEM_NOISE = 1e12
_CACHE = {}


def batch_of(case):
    """B = 3 to 5 over the cases."""
    return 3 + LP.CASES.index(case) % 3


class Stage:
    """Prior, the tangent of the same line, assembler and handle on ONE stream; the handle factored once on the assembler's
    pattern.  Carries what tests/test_gpu_burgers_prior.py::_check_ic_stage reads."""

    def __init__(self, pkg, cfg, B, ics=None, scheme="euler", analyse=True):
        import torch
        self.torch, self.pkg, self.cfg = torch, pkg, cfg
        self.ns, self.nt, self.B, self.dt = cfg.ns, cfg.nt, B, cfg.dt
        self.ics = LP.initial_conditions(pkg.workloads, cfg, B) if ics is None else ics
        self.stream = torch.cuda.Stream()
        s = self.stream.cuda_stream
        self.prior = cfg.prior(pkg, device=0, stream=s)
        self.tan = pkg.BurgersP1Tangent(cfg.ns, cfg.nt, cfg.dt, cfg.nu, stream=s, order=cfg.order, scheme=scheme, bc=cfg.bc,
                                        length=cfg.length)
        self.asm = pkg.PosteriorAssembler(self.prior.pattern, self.tan.pattern, stream=s)
        self.F = pkg.TridiagonalCholeskyFactor(stream=s, batch=B)
        if analyse:
            v = self.prior.values_batch(self.ics)
            x0 = np.repeat(v["bulk"][:, None], cfg.n, axis=1)
            x0[:, :cfg.ns] = self.ics
            jv, _ = self.tan.tangent_batch(x0)
            self.values0 = self.asm.precision_batch(v["q_values"], jv, FEM_NOISE)
            self.F.factor(self.asm.pattern, cfg.nt, values=self.values0)

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def matrix(self, q):
        P = self.prior.pattern
        return sp.csc_matrix((np.asarray(q), P.indices, P.indptr), shape=P.shape)


def reference(pkg, cfg, B, problems=None):
    """Computed once per case and left unchanged: the device's prior of the test batch and the oracle at the device's bulk[p]
    (of `problems` only, where given)."""
    key = (repr(cfg), B)
    problems = range(B) if problems is None else problems
    if key not in _CACHE:
        W = pkg.workloads
        ics = LP.initial_conditions(W, cfg, B)
        prior = cfg.prior(pkg, device=0)
        dev = prior.values_batch(ics)
        orc = {p: LP.oracle(W, cfg, float(dev["bulk"][p]), ics[p]) for p in problems}
        _CACHE[key] = types.SimpleNamespace(ics=ics, prior=prior, dev=dev, Q={p: o[0] for p, o in orc.items()},
                                            Qp={p: o[1] for p, o in orc.items()}, rhs={p: o[2] for p, o in orc.items()})
    return _CACHE[key]


@pytest.mark.parametrize("case", LP.CASES, ids=lambda c: "-".join(map(str, c)))
def test_bulk_values_and_information_vector_against_the_host_statement(pkg, case):
    cfg, B = LP.Cfg(*case), batch_of(case)
    r = reference(pkg, cfg, B)
    P, obs = r.prior.pattern, cfg.observed(pkg.workloads)
    assert r.prior.nnz == cfg.nnz()
    for p in range(B):
        ic, bulk = r.ics[p], float(r.dev["bulk"][p])
        e_bulk, tol_bulk = abs(bulk - ic[obs].mean()), LP.bulk_tol(cfg, ic)
        Qd = sp.csc_matrix((r.dev["q_values"][p], P.indices, P.indptr), shape=P.shape)
        ev = LP.value_excess(Qd, r.Q[p], cfg)
        er = LP.rhs_excess(r.dev["Qx_prior"][p], r.rhs[p], r.Qp[p], cfg, bulk, ic, pkg.workloads)
        print(f"{cfg} p={p}: bulk {bulk:+.3f} err {e_bulk:.2e} (tol {tol_bulk:.2e}); values at {ev:.4f} of the bound, Qx_prior at {er:.4f}")
        assert e_bulk <= tol_bulk
        assert ev <= 1.0 and er <= 1.0


@pytest.mark.parametrize("case", LP.CASES, ids=lambda c: "-".join(map(str, c)))
def test_values_are_symmetric_and_do_not_depend_on_the_batch(pkg, case):
    import torch
    cfg, B = LP.Cfg(*case), batch_of(case)
    r = reference(pkg, cfg, B)
    P, keys = r.prior.pattern, ("bulk", "q_values", "Qx_prior")
    for p in range(B):
        Qd = sp.csc_matrix((r.dev["q_values"][p], P.indices, P.indptr), shape=P.shape)
        assert abs(Qd - Qd.T).nnz == 0                                     # bitwise
        one = r.prior.values_batch(r.ics[p:p + 1])
        assert all(np.array_equal(one[k][0], r.dev[k][p]) for k in keys)
    perm = np.roll(np.arange(B), 1)[::-1].copy()
    other = r.prior.values_batch(r.ics[perm])
    assert all(np.array_equal(other[k], r.dev[k][perm]) for k in keys)
    again = r.prior.values_batch(r.ics)
    assert all(np.array_equal(again[k], r.dev[k]) for k in keys)
    on_dev = r.prior.values_batch(torch.from_numpy(r.ics).cuda())
    assert all(on_dev[k].is_cuda and np.array_equal(on_dev[k].cpu().numpy(), r.dev[k]) for k in keys)
    assert not np.array_equal(r.dev["q_values"][0], r.dev["q_values"][1])           # (the problems differ)


@pytest.mark.parametrize("ns,nt,B", [(64, 8, 5), (40, 5, 3)])
def test_p1_periodic_line_against_the_stencil_prior(pkg, ns, nt, B):
    """Two independent evaluations of one prior: the same pattern arrays, the same bulk bit for bit, values and Qx_prior within
    twice the bounds each is held to against the host statement."""
    cfg = LP.Cfg(1, "periodic", ns, nt)
    W = pkg.workloads
    ics = BP.initial_conditions(W, ns, B)
    line, stencil = cfg.prior(pkg, device=0), pkg.BurgersP1Prior(ns, nt, cfg.dt, cfg.nu, ic_noise=cfg.ic_noise)
    P, Ps = line.pattern, stencil.pattern
    assert np.array_equal(P.indptr, Ps.indptr) and np.array_equal(P.indices, Ps.indices)
    a, b = line.values_batch(ics), stencil.values_batch(ics)
    assert np.array_equal(a["bulk"], b["bulk"])
    for p in range(B):
        bulk = float(a["bulk"][p])
        Qa, Qb = (sp.csc_matrix((v["q_values"][p], P.indices, P.indptr), shape=P.shape) for v in (a, b))
        _, Qfree, _ = LP.oracle(W, cfg, bulk, ics[p])
        ev = LP.value_excess(Qa, Qb, cfg)
        er = LP.rhs_excess(a["Qx_prior"][p], b["Qx_prior"][p], Qfree, cfg, bulk, ics[p], W)
        print(f"{ns}x{nt} p={p}: line against stencil: values at {ev:.4f} of the bound, Qx_prior at {er:.4f}")
        assert ev <= 2.0 and er <= 2.0


@pytest.mark.parametrize("case", [(2, "periodic", 32, 8, "all"), (2, "dirichlet", 32, 6, "all")], ids=lambda c: "-".join(map(str, c)))
def test_ic_stage_against_a_sparse_lu(pkg, case):
    cfg, B = LP.Cfg(*case), 3
    r = reference(pkg, cfg, B)
    s = Stage(pkg, cfg, B, ics=r.ics)
    assert _check_ic_stage(pkg, s, r, range(B)) == 0           # blocks below 256 never carry the forward sweep
    s.torch.cuda.synchronize()


def test_ic_stage_takes_the_forward_in_factor_route_at_256_dofs(pkg, lib):
    """128 quadratic cells (ns = 256) x 6 slices as a batch of 16: whether the route qualifies is asked of the handle itself;
    where it does the stage must have taken it.  SciPy follows problems 0 and 5."""
    cfg, B = LP.Cfg(2, "periodic", 128, 6), 16
    r = reference(pkg, cfg, B, problems=(0, 5))
    s = Stage(pkg, cfg, B, ics=r.ics)
    probe = s.dev(r.dev["Qx_prior"])
    s.F.set_factor_rhs(probe)
    s.F.refactor(s.values0)
    state = C.c_int32(0)
    pkg._cabi.check(lib.gmrf_test_factor_fwd(s.F._h, C.byref(state), None))
    qualifies = state.value == 1
    s.F.set_factor_rhs(None)
    assert _check_ic_stage(pkg, s, r, (0, 5)) == (1 if qualifies else 0)
    pkg._cabi.check(lib.gmrf_test_factor_fwd(s.F._h, C.byref(state), None))
    assert state.value == 0                                     # (the run's registration does not outlive it)
    assert qualifies
    s.torch.cuda.synchronize()


def _single_loop(pkg, cfg, scheme, handed, p, n_steps):
    """tests/test_gpu_gn_batch.py::single_device_loop with the tangent of cfg's line: `gn_step` on a batch-1 handle."""
    import torch
    b = pkg.BurgersP1Tangent(cfg.ns, cfg.nt, cfg.dt, cfg.nu, order=cfg.order, scheme=scheme, bc=cfg.bc, length=cfg.length)
    Q = GO.problem_matrix(handed["Q"], handed["q_values"][p])
    asm = pkg.PosteriorAssembler(Q, b.pattern)
    qd, qx = torch.from_numpy(Q.data).cuda(), torch.from_numpy(handed["Qx_prior"][p]).cuda()
    x = torch.from_numpy(handed["x0"][p].copy()).cuda()
    F, out = None, []
    for _ in range(n_steps):
        jv, fv = b.tangent(x)
        if F is None:
            A = asm.pattern.copy(); A.data = asm.precision(qd, jv, handed["noise"]).cpu().numpy()
            F = pkg.tridiagonal_cholesky(A, cfg.nt)
        x = pkg.gn_step(F, asm, qd, qx, jv, x, -fv, handed["noise"])
        out.append(x.cpu().numpy().copy())
    return out


def test_chen24_hand_over_to_the_gauss_newton_loop(pkg):
    """BO.CHEN_CASE (32 quadratic cells x 26 slices, Crank-Nicolson, dirichlet, nu = 0.02, ic_noise 1e12) with the prior and x_ic
    from the device stage in the place of `burgers_chen24_batch`'s host prior and SuperLU solve: x_ic within `solve_tol` of the
    workload's x_prior; gn.run on the stage's device tensors takes the steps of the run on the workload's host inputs; its result
    by the rule of tests/test_gpu_burgers_prior.py::test_hand_over_to_the_gauss_newton_loop against tests/burgers_cn_oracle.py."""
    from tests.test_gpu_burgers_cn import Setup as HostSetup, device_rel_err
    c = BO.CHEN_CASE
    w, _, (xo, so, _, _, _) = BO.chen_case(pkg.workloads, "cn")
    cfg = LP.Cfg(c["order"], "dirichlet", c["nc"], c["nt"], nu=c["nu"], ic_noise=1e12, dt=w["dt"])
    assert cfg.ns == w["ns"] and cfg.length == w["length"]
    s = Stage(pkg, cfg, c["B"], ics=w["ic"], scheme="cn")
    ic_stage = pkg.BurgersInitialConditionBatch(s.F, s.asm, s.prior)
    gn = pkg.GaussNewtonBatch(s.F, s.asm, s.tan)
    x_ic, q, qx, bulk = ic_stage.run(s.dev(w["ic"]))
    assert x_ic.is_cuda and q.is_cuda and qx.is_cuda
    print("bulk", bulk.cpu().numpy())
    tol_ic = []
    for p in range(c["B"]):
        tol_ic.append(solve_tol(pkg.workloads.Workload("chen24_ic", w["Q"], w["Qx_prior"][p], cfg.nt, {})))
        e = rel(x_ic[p].cpu().numpy(), w["x_prior"][p])
        print(f"p={p}: x_ic against the workload's x_prior {e:.2e} (tol {tol_ic[p]:.2e})")
        assert e < tol_ic[p]
    x, steps, _ = gn.run(q, qx, x_ic, x_ic, noise=w["noise"], rtol=c["rtol"], max_steps=c["max_steps"])
    hs = HostSetup(pkg, w, "cn")
    _, steps_host, _ = hs.run(pkg.GaussNewtonBatch(hs.F, hs.asm, hs.tan), c["max_steps"], c["rtol"])
    print("steps", steps, "on the host inputs", steps_host, "oracle", so)
    assert np.array_equal(steps, steps_host)
    handed = {"Q": s.prior.pattern, "q_values": q.cpu().numpy(), "Qx_prior": qx.cpu().numpy(), "x0": x_ic.cpu().numpy(), "noise": w["noise"]}
    xn = x.cpu().numpy()
    for p in range(c["B"]):
        single = _single_loop(pkg, cfg, "cn", handed, p, int(steps[p]))
        e_b, e_s = rel(xn[p], xo[p]), rel(single[-1], xo[p])
        print(f"p={p} steps={int(steps[p])}: x batch {e_b:.2e} single {e_s:.2e} (x_ic's tolerance {tol_ic[p]:.2e}); "
              f"batch against single {rel(xn[p], single[-1]):.2e}")
        assert e_b <= 2 * e_s + 1e-12
        assert e_b < tol_ic[p]
    print("rel_err against Cole-Hopf at T = 1:", device_rel_err(pkg, w, x), "(README: 1.4e-3 / 3.8e-4 / 1.9e-3)")
    s.torch.cuda.synchronize()


def test_refusals_launch_nothing(pkg):
    cabi = pkg._cabi
    cfg, B = LP.Cfg(2, "periodic", 32, 8), 3
    s = Stage(pkg, cfg, B)

    def refused(fn, status=cabi.ERR_BAD_SHAPE):
        with pytest.raises(pkg.GmrfError) as e:
            fn()
        assert e.value.status == status and str(e.value).split(": ", 1)[1].strip()
    ic_stage = pkg.BurgersInitialConditionBatch(s.F, s.asm, s.prior)
    # a batch that is not the handle's
    refused(lambda: ic_stage.run(s.ics[:B - 1]))
    with pytest.raises(ValueError):
        ic_stage.run(s.ics[:, :-1])
    # a prior on another stream, a pattern-only prior
    refused(lambda: pkg.BurgersInitialConditionBatch(s.F, s.asm, cfg.prior(pkg, device=0)))
    refused(lambda: pkg.BurgersInitialConditionBatch(s.F, s.asm, cfg.prior(pkg, device=-1)), cabi.ERR_NO_DEVICE)
    refused(lambda: cfg.prior(pkg, device=-1).values_batch(s.ics), cabi.ERR_NO_DEVICE)
    # an assembler built on another line's prior pattern: the P1 periodic line with the same 64 dofs per slice
    other = LP.Cfg(1, "periodic", 64, 8).prior(pkg, device=0, stream=s.stream.cuda_stream)
    assert other.n == s.prior.n and other.nnz != s.prior.nnz
    blank = pkg.TridiagonalCholeskyFactor(stream=s.stream.cuda_stream, batch=B)
    refused(lambda: pkg.BurgersInitialConditionBatch(blank, s.asm, other))
    # ... and one of the same sizes: the dirichlet line's pattern with the pair (2, 0), (0, 2) moved to (cfg.ns - 1, 0), (0, cfg.ns - 1)
    dcfg = LP.Cfg(2, "dirichlet", 32, 6)
    dprior = dcfg.prior(pkg, device=0, stream=s.stream.cuda_stream)
    Pm = dprior.pattern.tolil()
    Pm[2, 0] = Pm[0, 2] = 0.0
    Pm[dcfg.ns - 1, 0] = Pm[0, dcfg.ns - 1] = 1.0
    moved = sp.csc_matrix(Pm)
    moved.eliminate_zeros()
    moved.sort_indices()
    assert moved.nnz == dprior.nnz
    dtan = pkg.BurgersP1Tangent(dcfg.ns, dcfg.nt, dcfg.dt, dcfg.nu, stream=s.stream.cuda_stream, order=2, bc="dirichlet", length=dcfg.length)
    refused(lambda: pkg.BurgersInitialConditionBatch(blank, pkg.PosteriorAssembler(moved, dtan.pattern, stream=s.stream.cuda_stream), dprior))
    # the stage still runs after the refusals
    x_ic = ic_stage.run(s.ics)[0]
    assert np.all(np.isfinite(x_ic))
    s.torch.cuda.synchronize()
