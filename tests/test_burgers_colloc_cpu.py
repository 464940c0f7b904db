"""The Burgers collocation tangent without a GPU: the library's pattern (device -1) and rejections, the restatement
tests/burgers_colloc_oracle.py checked by what its operators are, and the loop case COLLOC_CASE run on the restatement alone."""
import ctypes as C

import numpy as np
import pytest

from tests import burgers_colloc_oracle as CO

DT, NU = 0.05, 0.01
SHAPES = ((5, 3, 7), (20, 6, 27))          # (nc, nt, npts)


special_points = CO.special_points


@pytest.fixture(scope="module")
def case(pkg):
    """COLLOC_CASE on the oracle, computed once and left unchanged."""
    return CO.colloc_case(pkg.workloads)


def test_new_export_is_declared_everywhere(pkg, lib):
    name = "gmrf_burgers_colloc_create"
    assert name in pkg._cabi.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert issubclass(pkg.BurgersCollocationTangent, pkg.BurgersP1Tangent) and pkg.api.BurgersCollocationTangent is pkg.BurgersCollocationTangent


@pytest.mark.parametrize("nc,nt,npts", SHAPES)
def test_pattern_is_the_oracles(pkg, nc, nt, npts):
    """For J built with its explicit zeros: the point on 0.0 and the one on an inner vertex have a shape value that is exactly 0."""
    pts = special_points(nc, npts)
    b = pkg.BurgersCollocationTangent(nc, nt, DT, NU, pts, device=-1)
    _, J = CO.f_and_J(nc, nt, DT, NU, pts, np.random.default_rng(1).standard_normal(2 * nc * nt))
    assert (b.ns, b.order, b.scheme, b.bc) == (2 * nc, 2, "collocation", "periodic") and np.array_equal(b.points, pts)
    assert b.rows == (nt - 1) * npts and b.nnz == 6 * b.rows == J.nnz and b.n == 2 * nc * nt
    assert b.pattern.shape == J.shape == ((nt - 1) * npts, nt * 2 * nc)
    assert J.has_sorted_indices and np.array_equal(b.pattern.indptr, J.indptr) and np.array_equal(b.pattern.indices, J.indices)
    assert np.sum(J.data == 0.0) >= 2 * 2 * (nt - 1)            # (the stored zeros are there)
    # the wrap cell's row: columns (0, 2e, 2e+1) of each slice
    r = int(np.flatnonzero(pts == (nc - 1 + 0.65) * (1.0 / nc))[0])
    assert np.array_equal(J.indices[6 * r:6 * r + 6], [0, 2 * nc - 2, 2 * nc - 1, 2 * nc, 4 * nc - 2, 4 * nc - 1])


@pytest.mark.parametrize("nc,npts", [(5, 7), (20, 27), (200, 131)])
def test_operators_partition_of_unity(nc, npts):
    A, D1, D2 = CO.colloc_operators(nc, special_points(nc, npts), 1.0)
    one = np.ones(2 * nc)
    assert np.max(np.abs(A @ one - 1.0)) <= 1e-12 and np.max(np.abs(D1 @ one)) <= 1e-12 and np.max(np.abs(D2 @ one)) <= 1e-12


def test_operators_on_a_trigonometric_polynomial():
    """g = sin(2 pi x) + cos(4 pi x + 0.3) / 2 on nc = 200 cells.  With M3 = max |g'''| <= (2 pi)^3 + (4 pi)^3 / 2 and the
    quadratic interpolant Ig of a cell of length h: g - Ig = g'''(z) (x - x0)(x - xm)(x - x1) / 6, so |g - Ig| <= M3 h^3 / (72 sqrt 3).
    For the derivatives write g = q + R around the cell's midpoint, q quadratic (reproduced) and |R| <= M3 (h/2)^3 / 6,
    |R'| <= M3 (h/2)^2 / 2, |R''| <= M3 h / 2; R vanishes at the midpoint, so (IR)' and (IR)'' are sums over the two vertex
    shape functions, whose derivatives satisfy |phi_0'| + |phi_1'| <= 2 * 2/h and |phi_0''| + |phi_1''| = 2 * 4/h^2:
        |g' - (Ig)'| <= M3 h^2 (1/8 + 1/12),    |g'' - (Ig)''| <= M3 h (1/2 + 1/6)."""
    nc, length = 200, 1.0
    h = length / nc
    pts = special_points(nc, 131)
    A, D1, D2 = CO.colloc_operators(nc, pts, length)
    x = np.arange(2 * nc) * (h / 2)
    g = lambda x: np.sin(2 * np.pi * x) + 0.5 * np.cos(4 * np.pi * x + 0.3)
    g1 = lambda x: 2 * np.pi * np.cos(2 * np.pi * x) - 2 * np.pi * np.sin(4 * np.pi * x + 0.3)
    g2 = lambda x: -(2 * np.pi) ** 2 * np.sin(2 * np.pi * x) - 8 * np.pi ** 2 * np.cos(4 * np.pi * x + 0.3)
    M3 = (2 * np.pi) ** 3 + 0.5 * (4 * np.pi) ** 3
    e0, e1, e2 = (np.max(np.abs(A @ g(x) - g(pts))), np.max(np.abs(D1 @ g(x) - g1(pts))), np.max(np.abs(D2 @ g(x) - g2(pts))))
    b0, b1, b2 = M3 * h ** 3 / (72 * np.sqrt(3.0)), M3 * h ** 2 * (1 / 8 + 1 / 12), M3 * h * (1 / 2 + 1 / 6)
    print(f"value {e0:.2e} (bound {b0:.2e}), first derivative {e1:.2e} ({b1:.2e}), second {e2:.2e} ({b2:.2e})")
    assert e0 <= b0 and e1 <= b1 and e2 <= b2
    assert e1 > 1e-9 and e2 > 1e-6                 # (the data is not a quadratic: the bounds are not met trivially)


@pytest.mark.parametrize("nc,npts", [(5, 7), (16, 27)])
def test_operators_differentiate_polynomials_off_the_wrap_cell(nc, npts):
    """Away from the wrap cell the dof coordinates are a linear function along the cell: D1 x = 1 and D2 x^2 = 2 to 1e-12.
    Rounding: three terms of size <= (8 / h^2) x^2 with x < 1, each off by an ulp at most -- 3 * 8 * 16^2 * 1.1e-16 = 7e-13 at
    16 cells, which is why the mesh stops there."""
    pts = special_points(nc, npts)
    _, D1, D2 = CO.colloc_operators(nc, pts, 1.0)
    x = np.arange(2 * nc) / (2 * nc)
    inner = np.floor(pts * nc) < nc - 1
    assert 0 < inner.sum() < npts
    assert np.max(np.abs((D1 @ x)[inner] - 1.0)) <= 1e-12 and np.max(np.abs((D2 @ (x * x))[inner] - 2.0)) <= 1e-12
    assert np.min(np.abs((D1 @ x)[~inner] - 1.0)) > 0.1       # (the wrap cell sees the jump of the coordinate)


@pytest.mark.parametrize("nc,nt,npts", SHAPES)
def test_oracle_tangent_is_the_derivative_of_its_residual(nc, nt, npts):
    """f is quadratic in w, so (f(w + e v) - f(w - e v)) / 2e = J(w) v up to rounding."""
    rng = np.random.default_rng(3)
    pts = special_points(nc, npts)
    w = rng.standard_normal(2 * nc * nt)
    _, J = CO.f_and_J(nc, nt, DT, NU, pts, w)
    eps = 1e-3
    for _ in range(3):
        v = rng.standard_normal(w.size)
        fp, fm = CO.f_and_J(nc, nt, DT, NU, pts, w + eps * v)[0], CO.f_and_J(nc, nt, DT, NU, pts, w - eps * v)[0]
        jv = J @ v
        err = np.max(np.abs((fp - fm) / (2 * eps) - jv))
        print(f"{nc}x{nt}x{npts}: {err:.2e} of {np.max(np.abs(jv)):.2e}")
        assert err <= 1e-8 * np.max(np.abs(jv))


def test_bad_arguments_are_refused(pkg, lib):
    cabi = pkg._cabi

    def create(points, nc=5, nt=3, length=1.0, npts=None):
        p = np.ascontiguousarray(points, dtype=np.float64)
        h = C.c_void_p()
        st = lib.gmrf_burgers_colloc_create(-1, None, nc, nt, DT, NU, length, p.size if npts is None else npts, cabi.ptr(p), C.byref(h))
        if h.value:
            lib.gmrf_burgers_p1_destroy(h)
        return st, lib.gmrf_last_error().decode()

    good = [0.0, 0.3, 0.99]
    assert create(good)[0] == 0
    st, msg = create([0.1, 0.2, 1.0])                          # a point at `length`
    assert st == cabi.ERR_BAD_SHAPE and "point 2" in msg
    st, msg = create([0.1, -1e-9, 0.5])                        # a negative point
    assert st == cabi.ERR_BAD_SHAPE and "point 1" in msg
    st, msg = create([float("nan"), 0.2])                      # a NaN
    assert st == cabi.ERR_BAD_SHAPE and "point 0" in msg
    assert create(good, npts=0)[0] == cabi.ERR_BAD_SHAPE       # npts = 0
    assert create(good, nc=2)[0] == cabi.ERR_BAD_SHAPE         # nc = 2
    assert create([0.5, 1.5], length=2.0)[0] == 0 and create([0.5, 2.0], length=2.0)[0] == cabi.ERR_BAD_SHAPE
    # the line creator keeps rejecting the collocation scheme's value
    h = C.c_void_p()
    assert lib.gmrf_burgers_line_create(-1, None, 5, 3, DT, NU, 2, 2, 0, 1.0, C.byref(h)) == cabi.ERR_BAD_SHAPE and not h.value
    for bad in ([0.1, 1.0], [-0.5], [float("inf")], []):
        with pytest.raises(pkg.GmrfError) as e:
            pkg.BurgersCollocationTangent(5, 3, DT, NU, bad, device=-1)
        assert e.value.status == cabi.ERR_BAD_SHAPE
    with pytest.raises(pkg.GmrfError) as e:
        pkg.BurgersCollocationTangent(2, 3, DT, NU, good, device=-1)
    assert e.value.status == cabi.ERR_BAD_SHAPE
    with pytest.raises(pkg.GmrfError) as e:                    # the numeric phase needs the GPU: no CPU fallback
        pkg.BurgersCollocationTangent(5, 3, DT, NU, good, device=-1).tangent(np.zeros(30))
    assert e.value.status == cabi.ERR_NO_DEVICE


def test_workload(pkg):
    W, c = pkg.workloads, CO.COLLOC_CASE
    assert np.array_equal(W.burgers_collocation_points(np.arange(4) / 4, 5), np.linspace(0.2, 0.75 - 0.2, 5))
    w = W.burgers_collocation_batch(c["nc"], c["nt"], c["npts"], c["B"], c["nu"], c["T"], c["amp"])
    ns = 2 * c["nc"]
    assert (w["ns"], w["n"], w["m"], w["n_blocks"], w["dt"]) == (ns, ns * c["nt"], (c["nt"] - 1) * c["npts"], c["nt"], c["T"] / (c["nt"] - 1))
    assert w["q_values"].shape == (c["B"], w["Q"].nnz) and W.block_bandwidth_ok(w["Q"], c["nt"]) and abs(w["Q"] - w["Q"].T).max() == 0.0
    assert np.array_equal(w["ic"], c["amp"] * W.burgers_initial_conditions(ns, c["B"], 0)) and np.array_equal(w["x0"], w["x_prior"])
    assert np.array_equal(w["points"], W.burgers_collocation_points(np.arange(ns) / ns, c["npts"]))
    assert w["points"].shape == (c["npts"],) and w["points"].min() > 0.0 and w["points"].max() < 1.0
    assert not np.array_equal(w["q_values"][0], w["q_values"][1])
    for p in range(c["B"]):
        Q = CO.problem_matrix(w["Q"], w["q_values"][p])
        assert np.max(np.abs(Q @ w["x_prior"][p] - w["Qx_prior"][p])) < 1e-6 * np.max(np.abs(w["Qx_prior"][p]))
        assert np.max(np.abs(w["x0"][p, :ns] - w["ic"][p])) < 1e-3 * np.max(np.abs(w["ic"][p]))    # (observed with 1e8: the data dominates)
    asm = pkg.PosteriorAssembler(w["Q"], pkg.BurgersCollocationTangent(c["nc"], c["nt"], w["dt"], w["nu"], w["points"], device=-1).pattern,
                                 device=-1)
    assert (asm.n, asm.m) == (w["n"], w["m"]) and W.block_bandwidth_ok(asm.pattern, c["nt"])


def test_loop_case_on_the_oracle_alone(case):
    """COLLOC_CASE.  Measured: steps (4, 4, 5, 4, 4, 4), stop margin 5.5."""
    c = CO.COLLOC_CASE
    w, fJ, Qs, (x, steps, hist, rels, its) = case
    margin = CO.stop_margin(rels, c["rtol"])
    conds = [np.linalg.cond(CO.posterior_matrix(Qs[p], fJ(x[p])[1], w["noise"]).toarray()) for p in range(c["B"])]
    print("steps", steps, "stop margin", margin, "cond at the final iterates", conds)
    assert steps.max() < c["max_steps"]                        # every problem stops before max_steps
    assert len(set(steps.tolist())) >= 2                       # at least two different step counts
    assert margin >= 3.0
    assert len(its) == steps.max() and np.all(np.isfinite(x))
