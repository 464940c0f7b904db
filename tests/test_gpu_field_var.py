"""Pointwise predictive variance and calibration on the device (gmrf_eval_var_batch, gmrf_eval_calibration_batch,
`FieldEvaluator.variance` / `calibration`): the quadratic form against the selected inverse it reads, end to end against the dense
inverse in longdouble, determinism and plumbing, the calibration sums against longdouble NumPy, the refusals, and the Darcy loop's
end on device tensors.  Matrices, inverses and quadratic forms come from tests/field_var_oracle.py."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

from tests import field_eval_oracle as FO
from tests import field_var_oracle as VO
from tests.test_gpu_parity import solve_tol

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
# (geometry, nt, blocks): the periodic wrap cell in N = 3 blocks of 5; a two-slice quadratic line; P1 triangles with 2 vertex rows
# per block (bs = 10) and the 7 x 9 P2 lattice with 3 lattice rows per block (bs = 21), whose pairs cross block boundaries
CASES = [(("line", 5, 1, "periodic"), 3, 3), (("line", 4, 2, "dirichlet"), 2, 2), (("tri", 5, 6, 1), 1, 3), (("tri", 4, 5, 2), 1, 3)]
CASE_IDS = ["-".join(str(x) for x in c[0]) for c in CASES]
NPTS = (1, 257)
_cache = {}


def tol_sel(A):
    """What tests/test_gpu_selinv.py holds the selected inverse to, on the correlation scale."""
    return max(1e-10, 4.0 * solve_tol(SimpleNamespace(Q=sp.csc_matrix(A), meta={})))


def factor(pkg, geom, nt, nb, batch, seed=0, **kw):
    pattern, values, _ = VO.spd_matrix(geom, nt, batch, seed)
    F = pkg.TridiagonalCholeskyFactor(batch=batch, **kw)
    F.factor(pattern, nb, values=values)
    return F


def reference(geom, nt, batch, seed=0):
    """(Sigma_ref (batch, n, n) longdouble, tol_sel per problem), computed once per matrix."""
    key = ("ref", geom, nt, batch, seed)
    if key not in _cache:
        dense = VO.spd_matrix(geom, nt, batch, seed)[2]
        _cache[key] = (np.stack([VO.inverse_longdouble(d) for d in dense]), [tol_sel(d) for d in dense])
    return _cache[key]


def sigma_dense(K, vals):
    """The device's selected inverse on the pattern K as dense matrices (batch, n, n); zero where K stores nothing."""
    return np.stack([sp.csr_matrix((v, K.indices, K.indptr), shape=K.shape).toarray() for v in np.atleast_2d(vals)])


def device_results(pkg, case, batch):
    """Per npts: the rows, the variances on a device tensor and the selected inverse on pair_pattern(nt) taken separately."""
    import torch
    key = ("dev", case, batch)
    if key not in _cache:
        geom, nt, nb = case
        F = factor(pkg, geom, nt, nb, batch)
        res = {}
        for npts in NPTS:
            ev = VO.evaluator(pkg, geom, VO.points_of(geom)[-npts:])
            out = torch.empty((batch, nt, npts), dtype=torch.float64, device="cuda")
            assert ev.variance(F, nt, out=out) is out
            K = ev.pair_pattern(nt)
            vals = F.selected_inverse(pkg.CsrMatrix(K), out=np.empty((K.nnz,) if batch == 1 else (batch, K.nnz)))
            res[npts] = (ev.rows(), ev.ns, ev.width, out.cpu().numpy(), sigma_dense(K, vals))
            ev.close()
        F.close()
        _cache[key] = res
    return _cache[key]


def form_bound(W, mag):
    """Two nested W-term fma dot products: (2 W + 2) eps sum_ab |w_a w_b Sigma_ab|."""
    return (2 * W + 2) * EPS * mag


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_quadratic_form_against_the_selected_inverse_it_reads(pkg, case, batch):
    geom, nt, _ = case
    for npts, ((idx, w), ns, W, v, Sdev) in device_results(pkg, case, batch).items():
        assert v.shape == (batch, nt, npts)
        for p in range(batch):
            ref, mag = VO.quadratic_form(idx, w, nt, ns, Sdev[p])
            err, bound = np.abs(v[p].astype(np.longdouble) - ref), form_bound(W, mag)
            print(f"{geom} batch {batch} npts {npts} problem {p}: worst err / bound {float(np.max(err / bound)):.3f}")
            assert np.all(bound > 0) and np.all(err <= bound)
        if batch > 1:
            assert not np.array_equal(v[0], v[1])                              # (distinct values per problem)


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_variance_against_the_dense_inverse(pkg, case, batch):
    geom, nt, _ = case
    Sref, tols = reference(geom, nt, batch)
    for npts, ((idx, w), ns, W, v, _) in device_results(pkg, case, batch).items():
        for p in range(batch):
            ref, mag = VO.quadratic_form(idx, w, nt, ns, Sref[p])
            _, scale = VO.quadratic_form(idx, w, nt, ns, Sref[p], scale=np.sqrt(np.diag(Sref[p])))
            err, bound = np.abs(v[p].astype(np.longdouble) - ref), tols[p] * scale + form_bound(W, mag)
            print(f"{geom} batch {batch} npts {npts} problem {p}: tol_sel {tols[p]:.1e}, worst err / bound {float(np.max(err / bound)):.2e}, "
                  f"worst relative err {float(np.max(err / np.abs(ref))):.2e}")
            assert np.all(err <= bound) and np.all(v[p] > 0)


@pytest.mark.parametrize("case,batch", [(CASES[0], 1), (CASES[3], 3)], ids=[CASE_IDS[0], CASE_IDS[3]])
def test_determinism_and_plumbing(pkg, case, batch):
    import torch
    geom, nt, nb = case
    npts = 257
    F = factor(pkg, geom, nt, nb, batch)
    ev = VO.evaluator(pkg, geom, VO.points_of(geom)[-npts:])
    v = ev.variance(F, nt)
    assert isinstance(v, np.ndarray) and v.shape == (batch, nt, npts)
    assert np.array_equal(v, device_results(pkg, case, batch)[npts][3])         # another handle, another evaluator: the same bits
    assert np.array_equal(ev.variance(F, nt), v)                                # two calls
    dev = torch.empty((batch, nt, npts), dtype=torch.float64, device="cuda")
    host = np.empty((batch, nt, npts))
    assert ev.variance(F, nt, out=dev) is dev and ev.variance(F, nt, out=host) is host
    assert np.array_equal(dev.cpu().numpy(), v) and np.array_equal(host, v)     # host out, device out
    with pytest.raises(ValueError):
        ev.variance(F, nt, out=np.empty((batch, nt * npts + 1)))
    # std = sqrt(max(v, 0)), host and device
    assert np.array_equal(ev.variance(F, nt, std=True), np.sqrt(np.maximum(v, 0.0)))
    assert np.array_equal(ev.variance(F, nt, out=dev, std=True).cpu().numpy(), np.sqrt(np.maximum(v, 0.0)))
    # another pattern asked of the handle in between changes nothing
    A = VO.spd_matrix(geom, nt, batch)[0]
    F.selected_inverse(pkg.CsrMatrix(A), out=np.empty((A.nnz,) if batch == 1 else (batch, A.nnz)))
    assert np.array_equal(ev.variance(F, nt), v)
    F.marginal_var("exact")
    assert np.array_equal(ev.variance(F, nt), v)
    # new values on the same pattern: the evaluator's pattern matrix and the handle's plan stay (the handle counts no plan
    # builds, so the values are held to the end-to-end bound again)
    F.refactor(VO.spd_matrix(geom, nt, batch, 1)[1])
    v2 = ev.variance(F, nt)
    assert not np.array_equal(v2, v)
    Sref, tols = reference(geom, nt, batch, 1)
    (idx, w), W = ev.rows(), ev.width
    for p in range(batch):
        ref, mag = VO.quadratic_form(idx, w, nt, ev.ns, Sref[p])
        _, scale = VO.quadratic_form(idx, w, nt, ev.ns, Sref[p], scale=np.sqrt(np.diag(Sref[p])))
        assert np.all(np.abs(v2[p].astype(np.longdouble) - ref) <= tols[p] * scale + form_bound(W, mag))
    F.refactor(VO.spd_matrix(geom, nt, batch)[1])
    assert np.array_equal(ev.variance(F, nt), v)                                # back to the first values: the first bits
    ev.close(); F.close()


def sum_bound(terms, chain, count):
    """A sum of `count` terms as the device forms it -- a thread's chain, 8 tree levels in the workgroup, the chunks' chain and 8
    more levels in the finish launch -- of terms that each carry the division, the square root / log and the fma:
    (chain + 16 + 4) eps sum |terms| / count on the mean."""
    return (chain + 16 + 4) * EPS * float(np.sum(np.abs(terms))) / count


@pytest.mark.parametrize("first_slice", [0, 1])
def test_calibration_against_longdouble(pkg, first_slice):
    """Quadratic periodic line, nc = 16, nt = 4, batch 3, 700 points: 2800 / 2100 elements, no multiple of 256, two chunks."""
    import torch
    geom, nt, nb, B, npts, zcrit = ("line", 16, 2, "periodic"), 4, 4, 3, 700, 1.96
    F = factor(pkg, geom, nt, nb, B)
    ev = VO.evaluator(pkg, geom, VO.points_of(geom, n_random=700)[-npts:])
    rng = np.random.default_rng(12)
    fields = rng.uniform(-1.0, 1.0, (B, nt, ev.ns))
    pred, var = ev.apply(fields).reshape(B, nt * npts), ev.variance(F, nt).reshape(B, nt * npts)
    truth = pred + np.sqrt(var) * rng.standard_normal(pred.shape)               # z ~ N(0, 1) under the model
    first, n = first_slice * npts, nt * npts
    count = n - first
    nch = min(1024, max(1, (count + 2047) // 2048))
    length = (count + nch - 1) // nch
    chain = (length + 255) // 256 + (nch + 255) // 256
    assert count % 256 != 0 and nch == 2
    # longdouble reference from the device's pred and var and the truth
    pl, vl, tl = (a[:, first:].astype(np.longdouble) for a in (pred, var, truth))
    z = (pl - tl) / np.sqrt(vl)
    dens = -0.5 * (np.log(2 * np.longdouble(math.pi) * vl) + z * z)
    near = np.abs(np.abs(z) - zcrit) <= 1e-9 * zcrit
    assert near.sum() == 0                                                      # (seeded so: the count is then exact)
    want = np.stack([np.mean(z * z, axis=1), np.mean(np.abs(z) <= zcrit, axis=1), np.mean(dens, axis=1), vl.min(axis=1)], axis=1)

    out, pred_o, var_o = ev.calibration(F, fields, truth, nt=nt, first_slice=first_slice, zcrit=zcrit, return_pred=True, return_var=True)
    assert out.shape == (B, 4) and np.array_equal(pred_o, pred) and np.array_equal(var_o, var)
    for p in range(B):
        bz, bd = sum_bound(z[p] * z[p], chain, count), sum_bound(dens[p], chain, count)
        ez, ed = abs(np.longdouble(out[p, 0]) - want[p, 0]), abs(np.longdouble(out[p, 2]) - want[p, 2])
        cnt = int(np.sum(np.abs(z[p]) <= zcrit))
        print(f"first_slice {first_slice} problem {p}: out {out[p]}, mean z^2 err / bound {float(ez / bz):.3f}, "
              f"log density err / bound {float(ed / bd):.3f}, covered {cnt} of {count}")
        assert ez <= bz and ed <= bd
        assert round(out[p, 1] * count) == cnt and abs(out[p, 1] - cnt / count) <= EPS      # an integer count over count
        assert out[p, 3] == var[p, first:].min()                                # exact
    assert 0.85 < out[:, 1].min() and out[:, 1].max() < 0.995 and np.all(np.abs(out[:, 0] - 1.0) < 0.2)      # (z is standard normal)
    # the same bits on every call, without the extra outputs, and from device tensors
    assert np.array_equal(ev.calibration(F, fields, truth, nt=nt, first_slice=first_slice, zcrit=zcrit), out)
    fd, td = torch.from_numpy(fields).cuda(), torch.from_numpy(truth).cuda()
    out_d, pred_d, var_d = ev.calibration(F, fd.reshape(B, -1), td.reshape(B, nt, npts), nt=nt, first_slice=first_slice, zcrit=zcrit,
                                          return_pred=True, return_var=True)
    assert pred_d.is_cuda and var_d.is_cuda and np.array_equal(out_d, out)
    assert np.array_equal(pred_d.cpu().numpy(), pred) and np.array_equal(var_d.cpu().numpy(), var)
    out_v, var_only = ev.calibration(F, fd, td, nt=nt, first_slice=first_slice, zcrit=zcrit, return_var=True)
    assert np.array_equal(out_v, out) and np.array_equal(var_only.cpu().numpy(), var)
    # zcrit = 0 covers nobody, a huge one everybody; a zero variance shows in the fourth output
    assert np.all(ev.calibration(F, fd, td, nt=nt, first_slice=first_slice, zcrit=0.0)[:, 1] == 0.0)
    assert np.all(ev.calibration(F, fd, td, nt=nt, first_slice=first_slice, zcrit=1e300)[:, 1] == 1.0)
    ev.close(); F.close()


def test_refusals(pkg, lib):
    cabi = pkg._cabi
    w = pkg.workloads.make("darcy64")
    xy = np.array([[0.1, 0.2], [0.5, 0.5], [1.0, 1.0]])
    ev = pkg.FieldEvaluator.triangles(64, 64, xy, order=1)
    host_only = pkg.FieldEvaluator.triangles(64, 64, xy, order=1, device=-1)
    F = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
    fields, truth = np.zeros((1, w.n)), np.ones((1, 3))

    def refused(call, status, *words):
        with pytest.raises(cabi.GmrfError) as e:
            call()
        assert e.value.status == status, e.value
        for word in words:
            assert word in str(e.value), str(e.value)

    T = pkg.TridiagonalCholeskyFactor(order="twisted")
    T.factor(w.Q, w.n_blocks)
    refused(lambda: ev.variance(T), cabi.ERR_BAD_SHAPE, "twisted", "gmrf_eval_var_batch")
    refused(lambda: ev.calibration(T, fields, truth), cabi.ERR_BAD_SHAPE, "twisted", "gmrf_eval_calibration_batch")
    G = pkg.TridiagonalCholeskyFactor()
    refused(lambda: ev.variance(G), cabi.ERR_NO_FACTOR, "before factor")
    refused(lambda: ev.calibration(G, fields, truth), cabi.ERR_NO_FACTOR, "before factor")
    refused(lambda: ev.variance(F, nt=2), cabi.ERR_BAD_SHAPE, "nt * ns", str(w.n))
    refused(lambda: ev.calibration(F, np.zeros((1, 2 * w.n)), np.ones((1, 6)), nt=2), cabi.ERR_BAD_SHAPE, "nt * ns")
    refused(lambda: host_only.variance(F), cabi.ERR_NO_DEVICE)
    refused(lambda: host_only.calibration(F, fields, truth), cabi.ERR_NO_DEVICE)
    refused(lambda: ev.calibration(F, np.zeros((2, w.n)), np.ones((2, 3))), cabi.ERR_BAD_SHAPE, "batch")       # F holds one problem
    refused(lambda: ev.calibration(F, fields, truth, zcrit=-1.0), cabi.ERR_BAD_SHAPE, "zcrit")
    refused(lambda: ev.calibration(F, fields, truth, first_slice=1), cabi.ERR_BAD_SHAPE, "first_slice")
    out = np.empty(3)
    assert lib.gmrf_eval_var_batch(ev._h, F._h, 1, None) == cabi.ERR_BAD_SHAPE
    assert lib.gmrf_eval_var_batch(ev._h, None, 1, cabi.ptr(out)) == cabi.ERR_BAD_SHAPE
    assert lib.gmrf_eval_var_batch(None, F._h, 1, cabi.ptr(out)) == cabi.ERR_BAD_SHAPE
    # the handle and the evaluator still serve
    v = ev.variance(F)
    assert v.shape == (1, 1, 3) and np.all(v > 0)
    ev.close(); host_only.close(); T.close(); G.close(); F.close()


def test_the_darcy_loops_error_bars(pkg):
    """DarcyConditioningBatch(...).run(...) at batch 2 on workloads.darcy_conditioning(16)'s mesh, then the calibration of its mean
    on a 13 x 13 data grid that is not the node set, followed by mesh vertices: device tensors, one stream."""
    import torch
    from tests.test_gpu_darcy_batch import setup
    n_xy, B = 16, 2
    e = setup(pkg, n_xy, B)
    dc = pkg.DarcyConditioningBatch(e.F, e.asm, e.d)
    mean = dc.run(e.td, e.qd, k_samples=0, var=None).mean
    assert mean.is_cuda
    g = np.linspace(0.0, 1.0, 13)
    nodes = np.array([0, 5, 17, 100, 119, 255])                                 # dofs i + 16 j: corners, an edge, the interior
    vx = np.arange(n_xy) * (1.0 / (n_xy - 1))                                   # (vertex coordinates as field_eval_oracle.tri_points forms them)
    vx[-1] = 1.0
    verts = np.stack([vx[nodes % n_xy], vx[nodes // n_xy]], axis=1)
    xy = np.concatenate([pkg.workloads.darcy_pred_coords(g, g), verts])
    ev = pkg.FieldEvaluator.triangles(n_xy, n_xy, xy, order=1, stream=e.st.cuda_stream)
    idx, w = ev.rows()
    for k, node in enumerate(nodes):                  # those points coincide with their dofs (to the local coordinate's rounding)
        row = 169 + k
        assert np.max(np.abs(w[row] - (idx[row] == node))) <= 4 * n_xy * EPS
    truth = np.stack([np.sin(np.pi * xy[:, 0]) * np.sin(np.pi * xy[:, 1]) * (0.05 + 0.01 * p) for p in range(B)])
    out, var = ev.calibration(e.F, mean, torch.from_numpy(truth).cuda(), return_var=True)
    print("calibration (mean z^2, coverage, mean log density, min variance):", out, sep="\n")
    assert var.is_cuda and out.shape == (B, 4) and np.all(np.isfinite(out)) and np.all(out[:, 3] > 0)
    assert np.all((out[:, 1] >= 0) & (out[:, 1] <= 1))
    std = ev.variance(e.F, std=True).reshape(B, ev.npts)
    assert np.array_equal(std, np.sqrt(var.cpu().numpy()))
    mv = e.F.marginal_var("exact")
    nz = e.nz.cpu().numpy()
    for p in range(B):
        Qp = e.P.copy()
        Qp.data = nz[p].copy()
        tol = tol_sel(Qp)
        rel = np.abs(std[p, 169:] - np.sqrt(mv[p, nodes])) / np.sqrt(mv[p, nodes])
        print(f"problem {p}: std at the vertices against sqrt(marginal_var) rel {rel.max():.2e}, tol_sel {tol:.2e}")
        assert np.all(rel <= tol)
    ev.close(); dc.close(); e.F.close()
