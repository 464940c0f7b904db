"""Field evaluator (gmrf_eval_*, `FieldEvaluator`): what can be checked without a GPU, on handles created with device = -1 -- the
declarations, the rows of E against tests/field_eval_oracle.py, their structure, polynomial reproduction through `matrix()`, the
space-time stacking and the refused inputs."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from tests import field_eval_oracle as FO
from tests.test_host_logic import _check_julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["gmrf_eval_line_create", "gmrf_eval_tri_create", "gmrf_eval_destroy", "gmrf_eval_rows", "gmrf_eval_apply_batch",
               "gmrf_eval_errors_batch"]
EPS = 2.0 ** -52


def line_case(pkg, nc, order, bc, device=-1):
    length = FO.line_length(bc)
    pts = FO.line_points(nc, bc, length)
    return pkg.FieldEvaluator.line(nc, pts, order=order, bc=bc, length=length, device=device), pts, length


def tri_case(pkg, nx, ny, order, device=-1):
    xy = FO.tri_points(nx, ny)
    return pkg.FieldEvaluator.triangles(nx, ny, xy, order=order, device=device), xy


def test_new_exports_are_declared_everywhere(pkg, lib):
    hdr = open(os.path.join(ROOT, "include", "gmrf_hip.h")).read()
    shim = open(os.path.join(ROOT, "julia", "DiffEqGMRFsHIP.jl")).read()
    bound = _check_julia_ccalls(shim, hdr, 40)
    for name in NEW_EXPORTS:
        assert re.search(r"gmrf_status\s+%s\s*\(" % name, hdr), name
        assert name in pkg._cabi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
        assert name in bound, name
    assert "FieldEvaluator" in pkg.__all__
    for meth in ("line", "triangles", "rows", "matrix", "apply", "errors", "close"):
        assert hasattr(pkg.FieldEvaluator, meth)
    for fn in ("darcy_pred_coords", "burgers_pred_coords"):
        assert hasattr(pkg.workloads, fn)
    assert "field_eval.hpp" in open(os.path.join(ROOT, "diffeqgmrfs.jl_amd", "csrc", "Makefile")).read()


def test_pred_coords_follow_the_scripts_order(pkg):
    xs, ys = np.array([0.0, 0.5, 1.0]), np.array([0.25, 0.75])
    xy = pkg.workloads.darcy_pred_coords(xs, ys)
    assert xy.shape == (6, 2) and xy.flags.c_contiguous
    assert np.array_equal(xy, [[x, y] for x in xs for y in ys])              # x outer, y inner
    assert np.array_equal(pkg.workloads.burgers_pred_coords(xs), xs)


def _check_rows(ev, idx_o, w_o, ns, width):
    idx, w = ev.rows()
    assert (ev.ns, ev.width, ev.npts) == (ns, width, idx_o.shape[0])
    assert idx.dtype == np.int64 and idx.shape == w.shape == (ev.npts, width)
    assert np.array_equal(idx, idx_o)
    ulps = np.max(np.abs(w - w_o) / np.spacing(np.abs(w_o)))
    print(f"rows: max |w - oracle| = {ulps:.1f} ulp")
    assert ulps <= 4.0
    # structure: ascending, in range, a partition of unity
    assert np.all(np.diff(idx, axis=1) > 0) and idx.min() >= 0 and idx.max() < ns
    assert np.max(np.abs(w.sum(axis=1) - 1.0)) <= 4 * EPS
    return idx, w


@pytest.mark.parametrize("nc,order,bc", FO.LINES)
def test_line_rows_against_the_oracle(pkg, nc, order, bc):
    ev, pts, length = line_case(pkg, nc, order, bc)
    idx_o, w_o = FO.line_rows(nc, order, bc, length, pts)
    idx, w = _check_rows(ev, idx_o, w_o, FO.line_ns(nc, order, bc), order + 1)
    # a point on a vertex (point 300 + k is vertex k): weight 1.0 there, explicit zeros beside it
    for k in (0, 1, nc - 1):
        row = 300 + k
        assert w[row, list(idx[row]).index(order * k)] == 1.0 and np.count_nonzero(w[row] == 0.0) == order
    if bc == "periodic":
        assert idx[-1, 0] == 0 and idx[-1, -1] == ev.ns - 1          # the largest double below length: the wrap cell, dof 0
        assert np.max(np.abs(w[-1] - (np.arange(order + 1) == 0))) <= 4 * nc * EPS       # (1 - xi = nc eps there)
    else:
        assert idx[-1, -1] == ev.ns - 1 and abs(w[-1, -1] - 1.0) <= 4 * nc * EPS          # x = length on the interval: the last cell
    ev.close()
    ev.close()                                                        # (closing twice is fine)


@pytest.mark.parametrize("nx,ny,order", FO.TRIANGLES)
def test_triangle_rows_against_the_oracle(pkg, nx, ny, order):
    ev, xy = tri_case(pkg, nx, ny, order)
    idx_o, w_o = FO.tri_rows(nx, ny, order, xy)
    idx, w = _check_rows(ev, idx_o, w_o, FO.tri_ns(nx, ny, order), 3 if order == 1 else 6)
    lx = nx if order == 1 else 2 * nx - 1
    # a point on a vertex (point 300 + i + nx j is vertex (i, j)): weight 1.0 at its dof, explicit zeros for the rest
    for i, j in ((0, 0), (1, 2), (nx - 1, ny - 1), (nx - 1, 0), (0, ny - 1)):
        row = 300 + i + nx * j
        assert w[row, list(idx[row]).index(order * (i + lx * j))] == 1.0 and np.count_nonzero(w[row] == 0.0) == ev.width - 1
    # t == s exactly goes to the lower triangle (n00, n10, n11) of quad (0, 0): dof of n10 is in the row, that of n01 is not
    for row in (300 + nx * ny, 301 + nx * ny):
        assert order * 1 in idx[row] and order * lx not in idx[row]
    ev.close()


def _poly_line(coef, x):
    return sum(c * x ** k for k, c in enumerate(coef))


def _poly_tri(coef, order, x, y):
    terms = [(i, j) for i in range(order + 1) for j in range(order + 1 - i)]
    return sum(c * x ** i * y ** j for c, (i, j) in zip(coef, terms))


def _reproduction_bound(E, f, m):
    return EPS * (8.0 * (abs(E) @ np.abs(f)) + 64.0 * m * np.max(np.abs(f)))


@pytest.mark.parametrize("nc,order", [(nc, order) for nc in (4, 5, 16) for order in (1, 2)])
def test_line_reproduces_polynomials(pkg, nc, order):
    """A polynomial of degree <= order sampled at the dofs and evaluated through matrix() is the polynomial at the points, within
    eps (8 sum |w||f| + 64 nc max |f|): the dot product's and the weights' rounding, and the local coordinate's (|d xi| <~ 2 eps /
    h times the weights' slopes).  A wrong cell, local order or index is wrong by O(h^2) >= 1e-3.  On the interval: a periodic
    field is no polynomial across the wrap."""
    ev, pts, length = line_case(pkg, nc, order, "dirichlet")
    E = ev.matrix()
    assert E.shape == (ev.npts, ev.ns) and E.nnz == ev.npts * ev.width
    rng = np.random.default_rng(nc + order)
    for _ in range(4):
        coef = rng.uniform(-1.0, 1.0, order + 1)
        f = _poly_line(coef, FO.line_dof_coords(nc, order, "dirichlet", length))
        exact = _poly_line(coef.astype(np.longdouble), pts.astype(np.longdouble))
        err, bound = np.abs((E @ f).astype(np.longdouble) - exact), _reproduction_bound(E, f, nc)
        print(f"nc={nc} order={order}: max err {float(err.max()):.2e}, worst err / bound {float(np.max(err / bound)):.3f}")
        assert np.all(err <= bound)


@pytest.mark.parametrize("nx,ny,order", FO.TRIANGLES)
def test_triangles_reproduce_polynomials(pkg, nx, ny, order):
    """As on the line, with total degree <= order in (x, y) and m = max(nx, ny) - 1.  (3, 4) and (5, 3): a swapped x / y cannot
    pass on a mesh that is not square."""
    ev, xy = tri_case(pkg, nx, ny, order)
    E = ev.matrix()
    assert E.shape == (ev.npts, ev.ns) and E.nnz == ev.npts * ev.width
    dofs = FO.tri_dof_coords(nx, ny, order)
    xl, yl = xy[:, 0].astype(np.longdouble), xy[:, 1].astype(np.longdouble)
    rng = np.random.default_rng(nx * ny + order)
    for _ in range(4):
        coef = rng.uniform(-1.0, 1.0, (order + 1) * (order + 2) // 2)
        f = _poly_tri(coef, order, dofs[:, 0], dofs[:, 1])
        exact = _poly_tri(coef.astype(np.longdouble), order, xl, yl)
        err, bound = np.abs((E @ f).astype(np.longdouble) - exact), _reproduction_bound(E, f, max(nx, ny) - 1)
        print(f"{nx}x{ny} order={order}: max err {float(err.max()):.2e}, worst err / bound {float(np.max(err / bound)):.3f}")
        assert np.all(err <= bound)


def test_matrix_stacks_the_slices(pkg):
    ev, _, _ = line_case(pkg, 5, 2, "periodic")
    E = ev.matrix()
    idx, w = ev.rows()
    assert np.array_equal(E.indices.reshape(ev.npts, ev.width), idx) and np.array_equal(E.data.reshape(ev.npts, ev.width), w)
    E3 = ev.matrix(nt=3)
    assert E3.shape == (3 * ev.npts, 3 * ev.ns) and E3.nnz == 3 * E.nnz            # (explicit zeros kept)
    K = sp.kron(sp.identity(3), E, format="csr")
    assert abs(E3 - K).max() == 0.0
    A_ic = ev.matrix(nt=3, slice=0)
    assert A_ic.shape == (ev.npts, 3 * ev.ns) and A_ic.indices.max() < ev.ns and abs(A_ic[:, :ev.ns] - E).max() == 0.0
    A_2 = ev.matrix(nt=3, slice=2)
    assert A_2.indices.min() >= 2 * ev.ns and abs(A_2 - E3[2 * ev.npts:]).max() == 0.0
    with pytest.raises(ValueError):
        ev.matrix(nt=3, slice=3)


def test_numeric_calls_need_the_device(pkg):
    ev, _, _ = line_case(pkg, 4, 1, "periodic")
    for call in (lambda: ev.apply(np.zeros((2, ev.ns))), lambda: ev.errors(np.zeros((2, ev.ns)), np.ones((2, ev.npts)))):
        with pytest.raises(pkg.GmrfError) as e:
            call()
        assert e.value.status == pkg._cabi.ERR_NO_DEVICE


def test_refused_inputs(pkg, lib):
    FE, bad = pkg.FieldEvaluator, pkg._cabi.ERR_BAD_SHAPE
    ok = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6])
    sq = np.array([[0.1, 0.2], [0.3, 0.4], [0.5, 0.6], [0.7, 0.8]])

    def refused(make, *words):
        with pytest.raises(pkg.GmrfError) as e:
            make()
        assert e.value.status == bad, e.value
        for word in words:
            assert word in str(e.value), str(e.value)

    refused(lambda: FE.line(4, ok, order=3, device=-1), "order")
    refused(lambda: FE.line(4, ok, order=0, device=-1), "order")
    refused(lambda: FE.line(4, ok, bc="neumann", device=-1), "bc")
    h = C.c_void_p()
    st = lib.gmrf_eval_line_create(-1, None, 4, 2, 7, 1.0, ok.size, pkg._cabi.ptr(ok), C.byref(h))      # a bc the C ABI does not know
    assert st == bad and not h.value and b"bc" in lib.gmrf_last_error()
    refused(lambda: FE.line(4, ok, length=0.0, device=-1), "length")
    refused(lambda: FE.line(4, ok, length=-1.0, device=-1), "length")
    refused(lambda: FE.line(2, ok, bc="periodic", device=-1), "nc")
    refused(lambda: FE.line(1, ok, bc="dirichlet", device=-1), "nc")
    FE.line(3, ok, bc="periodic", device=-1).close()
    FE.line(2, ok, bc="dirichlet", device=-1).close()
    refused(lambda: FE.line(4, np.zeros(0), device=-1), "npts")
    refused(lambda: FE.triangles(1, 4, sq, device=-1), "nx")
    refused(lambda: FE.triangles(4, 1, sq, device=-1), "ny")
    refused(lambda: FE.triangles(4, 4, sq, order=3, device=-1), "order")
    refused(lambda: FE.triangles(4, 4, np.zeros((0, 2)), device=-1), "npts")
    # points: not finite, outside the domain -- the message names the first offending index
    for k, v in ((4, np.nan), (2, np.inf), (5, -1e-300), (3, 1.0), (1, 1.5)):
        pts = ok.copy()
        pts[k] = v
        refused(lambda: FE.line(4, pts, bc="periodic", device=-1), f"point {k} ")
    pts = 2.0 * ok
    pts[3] = np.nextafter(2.0, 3.0)
    refused(lambda: FE.line(4, pts, bc="dirichlet", length=2.0, device=-1), "point 3 ")
    pts[3] = 2.0
    FE.line(4, pts, bc="dirichlet", length=2.0, device=-1).close()
    pts[3], pts[5] = -0.5, np.nan                                      # two offenders: the first one is named
    refused(lambda: FE.line(4, pts, bc="dirichlet", length=2.0, device=-1), "point 3 ")
    for (k, c), v in (((2, 0), np.nan), ((1, 1), np.inf), ((3, 0), np.nextafter(1.0, 2.0)), ((0, 1), -1e-300), ((2, 1), 1.5)):
        xy = sq.copy()
        xy[k, c] = v
        refused(lambda: FE.triangles(4, 5, xy, device=-1), f"point {k} ")
    sq[1] = (1.0, 1.0)
    FE.triangles(4, 5, sq, order=2, device=-1).close()
    with pytest.raises(ValueError):
        FE.triangles(4, 5, np.zeros((4, 3)), device=-1)
