"""Field evaluator on the device (gmrf_eval_apply_batch, gmrf_eval_errors_batch, `FieldEvaluator`): `apply` against the handle's own
rows in longdouble, its determinism, the fused metrics against `apply` + `solution_errors_batch` bit for bit, and the last line of
the Darcy and the Burgers data-set loops on device tensors."""
import ctypes as C

import numpy as np
import pytest

from tests import field_eval_oracle as FO

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
GEOMETRIES = [("line",) + g for g in FO.LINES] + [("tri",) + g for g in FO.TRIANGLES]
NPTS = (1, 255, 257, 700)           # a partial workgroup, one short of / one past a workgroup, no multiple of anything
ROWS = (1, 3, 5)


def make(pkg, geom, npts, **kw):
    """The evaluator of a geometry on the LAST npts of its test points (700 random ones, then the corner cases)."""
    if geom[0] == "line":
        _, nc, order, bc = geom
        length = FO.line_length(bc)
        pts = FO.line_points(nc, bc, length, n_random=700)[-npts:]
        return pkg.FieldEvaluator.line(nc, pts, order=order, bc=bc, length=length, **kw)
    _, nx, ny, order = geom
    return pkg.FieldEvaluator.triangles(nx, ny, FO.tri_points(nx, ny, n_random=700)[-npts:], order=order, **kw)


def check_apply(ev, fields, pred):
    """|pred - sum w f| <= (width + 1) eps sum |w||f|: the bound of a width-term dot product; the weights are shared."""
    idx, w = ev.rows()
    ref, mag = FO.dot_rows(idx, w, fields)
    err, bound = np.abs(pred.astype(np.longdouble) - ref), (ev.width + 1) * EPS * mag
    worst = float(np.max(err / np.where(bound > 0, bound, 1)))
    assert np.all(err <= bound), worst
    return worst


@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: "-".join(str(x) for x in g))
def test_apply_against_the_rows_in_longdouble(pkg, geom):
    import torch
    rng = np.random.default_rng(7)
    worst = 0.0
    for npts in NPTS:
        ev = make(pkg, geom, npts)
        assert ev.npts == npts
        F5 = rng.uniform(-1.0, 1.0, (5, ev.ns))
        P5 = ev.apply(F5)
        assert P5.shape == (5, npts)
        for rows in ROWS:
            P = ev.apply(F5[:rows])
            worst = max(worst, check_apply(ev, F5[:rows], P))
            assert np.array_equal(P, P5[:rows])                                  # (the same bits for every `rows`)
        for r in range(5):                                                      # row r of a call is the one-row call on it
            assert np.array_equal(ev.apply(F5[r]), P5[r])
        assert np.array_equal(ev.apply(F5), P5)                                  # ... and on every call
        Pd = ev.apply(torch.from_numpy(F5).cuda())                               # device pointers: the same bits
        assert Pd.is_cuda and np.array_equal(Pd.cpu().numpy(), P5)
        assert np.array_equal(ev.apply(F5.reshape(5, 1, ev.ns)).reshape(5, npts), P5)       # (any leading shape)
        ev.close()
    print(f"{geom}: worst err / bound {worst:.3f}")


def test_apply_loops_over_more_rows_than_a_grid_dimension_holds(pkg):
    """rows = 65 537 on the nc = 4 P1 periodic line with 3 points: 2 MB in, one row more than gridDim.y can hold twice over."""
    rows = 65537
    ev = pkg.FieldEvaluator.line(4, np.array([0.3, np.nextafter(1.0, 0.0), 0.5]), order=1, bc="periodic")
    F = np.random.default_rng(8).uniform(-1.0, 1.0, (rows, ev.ns))
    P = ev.apply(F)
    print(f"rows={rows}: worst err / bound {check_apply(ev, F, P):.3f}")
    assert np.array_equal(P[-1], ev.apply(F[-1])) and np.array_equal(P[65535], ev.apply(F[65535]))
    ev.close()


def host_errors(pkg, pred, truth, first):
    e = [pkg.workloads.solution_errors(p[first:], t[first:]) for p, t in zip(pred, truth)]
    return np.array([[d["rel_err"], d["rmse"], d["max_err"]] for d in e])


@pytest.mark.parametrize("geom", [("line", 16, 1, "periodic"), ("line", 16, 2, "dirichlet"), ("tri", 17, 9, 2)],
                         ids=lambda g: "-".join(str(x) for x in g))
def test_fused_errors_are_apply_then_solution_errors_bitwise(pkg, geom):
    """nt = 4, first_slice = 1 at 700 points: 2100 elements, two chunks of the metrics' partition."""
    import torch
    ev = make(pkg, geom, 700)
    rng = np.random.default_rng(9)
    for B in (1, 3):
        for nt in (1, 4):
            F = rng.uniform(-1.0, 1.0, (B, nt, ev.ns))
            P = ev.apply(F).reshape(B, nt * ev.npts)
            T = P + 1e-3 * rng.standard_normal(P.shape)
            for first_slice in range(min(nt, 2)):
                first = first_slice * ev.npts
                want = pkg.solution_errors_batch(P, T, first=first)
                got = ev.errors(F, T, nt=nt, first_slice=first_slice)
                assert got.shape == (B, 3) and np.array_equal(got, want), (B, nt, first_slice, got, want)
                got_p, pred = ev.errors(F.reshape(B, -1), T.reshape(B, nt, ev.npts), nt=nt, first_slice=first_slice, return_pred=True)
                assert np.array_equal(got_p, want) and np.array_equal(pred, P)
                got_d, pred_d = ev.errors(torch.from_numpy(F).cuda(), torch.from_numpy(T).cuda(), nt=nt, first_slice=first_slice,
                                          return_pred=True)
                assert pred_d.is_cuda and np.array_equal(got_d, want) and np.array_equal(pred_d.cpu().numpy(), P)
                assert np.array_equal(ev.errors(torch.from_numpy(F).cuda(), torch.from_numpy(T).cuda(), nt=nt, first_slice=first_slice), want)
                ref = host_errors(pkg, P, T, first)
                rel = np.max(np.abs(got - ref) / np.abs(ref))
                print(f"{geom} B={B} nt={nt} first_slice={first_slice}: device vs host metrics rel {rel:.2e}")
                assert rel <= 1e-13
            if nt == 1:
                with pytest.raises(pkg.GmrfError) as e:                           # first_slice = 1 leaves nothing of one slice
                    ev.errors(F, T, nt=1, first_slice=1)
                assert e.value.status == pkg._cabi.ERR_BAD_SHAPE
    ev.close()


def check_loop_end(pkg, ev, fields_d, truth, nt, first_slice):
    """errors / pred of device tensors against the host composition matrix() @ field + NumPy metrics.  The device's pred and the
    host's each lie within delta = (width + 1) eps sum |w||f| of the longdouble sum (check_apply: a double dot product of width
    terms, fused or not), so they differ by 2 delta at the most; a metric moves by at most max 2 delta (rmse, max_err) or
    |2 delta| / |truth| (rel_err) with pred, and by 1e-13 of itself with the order of its sums."""
    import torch
    B = fields_d.shape[0]
    truth_d = torch.from_numpy(truth).cuda()
    got, pred = ev.errors(fields_d, truth_d, nt=nt, first_slice=first_slice, return_pred=True)
    assert pred.is_cuda and np.array_equal(got, ev.errors(fields_d, truth_d, nt=nt, first_slice=first_slice))
    f_host = fields_d.cpu().numpy().reshape(B, -1)
    E = ev.matrix(nt=nt)
    pred_h = (E @ f_host.T).T
    delta = (ev.width + 1) * EPS * (abs(E) @ np.abs(f_host).T).T
    slices = f_host.reshape(B, nt, ev.ns)
    print(f"pred: device err / bound {check_apply(ev, slices, pred.cpu().numpy().reshape(B, nt, ev.npts)):.3f}, "
          f"host err / bound {check_apply(ev, slices, pred_h.reshape(B, nt, ev.npts)):.3f}")
    first = first_slice * ev.npts
    ref = host_errors(pkg, pred_h, truth, first)
    d = 2 * delta[:, first:]
    slack = np.stack([np.linalg.norm(d, axis=1) / np.linalg.norm(truth[:, first:], axis=1), d.max(axis=1), d.max(axis=1)], axis=1)
    print("device", got, "host", ref, "slack", slack, sep="\n")
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - ref) <= slack + 1e-13 * np.abs(ref))
    return got


def test_the_darcy_loops_last_line(pkg):
    """DarcyConditioningBatch(...).run(...).mean at batch 2 on the 64 x 64 mesh, evaluated on a 13 x 13 data grid that is not the
    node set and compared with a truth there: device tensors end to end, one stream."""
    from tests.test_gpu_darcy_batch import setup
    e = setup(pkg, 64, 2)
    dc = pkg.DarcyConditioningBatch(e.F, e.asm, e.d)
    mean = dc.run(e.td, e.qd, k_samples=0, var=None).mean
    assert mean.is_cuda
    g = np.linspace(0.0, 1.0, 13)
    xy = pkg.workloads.darcy_pred_coords(g, g)
    ev = pkg.FieldEvaluator.triangles(64, 64, xy, order=1, stream=e.st.cuda_stream)
    assert (ev.ns, ev.npts) == (e.n, 169)
    truth = np.stack([np.sin(np.pi * xy[:, 0]) * np.sin(np.pi * xy[:, 1]) * (0.05 + 0.01 * p) for p in range(2)])
    check_loop_end(pkg, ev, mean, truth, 1, 0)
    ev.close(); dc.close(); e.F.close()


def test_the_burgers_loops_last_line(pkg):
    """The final iterates of GaussNewtonBatch on tests/gn_batch_oracle.py's GN_CASE (64 nodes x 8 slices, 6 problems), evaluated
    slice by slice on 100 points between the nodes, the first slice left out as the scripts' [2:end, :] does."""
    from tests import gn_batch_oracle as GO
    from tests.test_gpu_gn_batch import Setup
    c = GO.GN_CASE
    s = Setup(pkg, c["ns"], c["nt"], c["B"], seed=c["seed"])
    gn = pkg.GaussNewtonBatch(s.F, s.asm, s.tan)
    w = s.w
    x, steps, _ = gn.run(s.dev(w["q_values"]), s.dev(w["Qx_prior"]), s.dev(w["x_prior"]), s.dev(w["x0"]), noise=s.noise,
                         rtol=c["rtol"], max_steps=c["max_steps"])
    assert x.is_cuda and tuple(x.shape) == (c["B"], c["ns"] * c["nt"])
    pts = pkg.workloads.burgers_pred_coords((np.arange(100) + 0.5) / 100.0)
    ev = pkg.FieldEvaluator.line(c["ns"], pts, order=1, bc="periodic", stream=s.stream.cuda_stream)
    assert (ev.ns, ev.npts) == (c["ns"], 100)
    rng = np.random.default_rng(10)
    truth = (ev.matrix(nt=c["nt"]) @ w["x_prior"].T).T + 1e-2 * rng.standard_normal((c["B"], c["nt"] * 100))
    got = check_loop_end(pkg, ev, x, truth, c["nt"], 1)
    assert not np.array_equal(got, ev.errors(x, s.dev(truth), nt=c["nt"], first_slice=0))           # (the first slice counts)
    ev.close(); gn.close(); s.F.close()


def test_refusals(pkg, lib):
    cabi = pkg._cabi
    pts = np.array([0.1, 0.6, 0.35])
    host_only = pkg.FieldEvaluator.line(4, pts, order=2, device=-1)
    ev = pkg.FieldEvaluator.line(4, pts, order=2)
    F, T = np.zeros((2, 3, ev.ns)), np.ones((2, 3, ev.npts))
    for call in (lambda: host_only.apply(F), lambda: host_only.errors(F, T, nt=3)):
        with pytest.raises(pkg.GmrfError) as e:
            call()
        assert e.value.status == cabi.ERR_NO_DEVICE

    def bad(status):
        assert status == cabi.ERR_BAD_SHAPE and lib.gmrf_last_error()

    out, pred = np.empty((2, 3)), np.empty((2, 3, ev.npts))
    p = cabi.ptr
    bad(lib.gmrf_eval_errors_batch(ev._h, 0, 3, 0, p(F), p(T), p(out), None))            # batch in [1, 4096]
    bad(lib.gmrf_eval_errors_batch(ev._h, 4097, 3, 0, p(F), p(T), p(out), None))
    bad(lib.gmrf_eval_errors_batch(ev._h, 2, 0, 0, p(F), p(T), p(out), None))            # nt >= 1
    bad(lib.gmrf_eval_errors_batch(ev._h, 2, 3, 3, p(F), p(T), p(out), None))            # 0 <= first_slice < nt
    bad(lib.gmrf_eval_errors_batch(ev._h, 2, 3, -1, p(F), p(T), p(out), None))
    bad(lib.gmrf_eval_errors_batch(ev._h, 2, 3, 0, None, p(T), p(out), None))            # null fields, truth, errors_out
    bad(lib.gmrf_eval_errors_batch(ev._h, 2, 3, 0, p(F), None, p(out), None))
    bad(lib.gmrf_eval_errors_batch(ev._h, 2, 3, 0, p(F), p(T), None, p(pred)))
    bad(lib.gmrf_eval_apply_batch(ev._h, 0, p(F), p(pred)))                              # rows in [1, 2^24]
    bad(lib.gmrf_eval_apply_batch(ev._h, (1 << 24) + 1, p(F), p(pred)))
    bad(lib.gmrf_eval_apply_batch(ev._h, 6, None, p(pred)))
    bad(lib.gmrf_eval_apply_batch(ev._h, 6, p(F), None))
    bad(lib.gmrf_eval_apply_batch(None, 6, p(F), p(pred)))
    with pytest.raises(ValueError):
        ev.apply(np.zeros((2, ev.ns + 1)))
    with pytest.raises(ValueError):
        ev.errors(F, T, nt=2)
    assert lib.gmrf_eval_errors_batch(ev._h, 2, 3, 2, p(F), p(T), p(out), p(pred)) == cabi.GMRF_OK and np.all(pred == 0.0)
    assert np.array_equal(out, np.tile([1.0, 1.0, 1.0], (2, 1)))                         # (pred 0 against truth 1)
    ev.close(); host_only.close()
