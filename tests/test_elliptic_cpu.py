"""Nonlinear elliptic tangent and its Gauss-Newton loop: what can be checked without a GPU (declarations, the pattern-only
handle, argument validation, the NumPy oracle's own consistency and the conditioning of the GPU test's inputs)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import elliptic_oracle as EO
from tests import gn_batch_oracle as GO
from tests.test_host_logic import _check_julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["gmrf_elliptic_p1_create", "gmrf_elliptic_p1_destroy", "gmrf_elliptic_p1_pattern", "gmrf_elliptic_p1_qpoints",
               "gmrf_elliptic_p1_tangent", "gmrf_elliptic_p1_tangent_batch", "gmrf_elliptic_p1_load", "gmrf_gn_create_elliptic"]
MESHES = ((3, 3), (16, 16), (19, 14))


@pytest.fixture(scope="module")
def gn_cases(pkg):
    """EO.GN_CASE on both meshes, computed once: mesh -> (workload, Problem, batch_loop result)."""
    return {ms: EO.oracle_case(pkg.workloads, ms) for ms in EO.GN_CASE["meshes"]}


def test_new_exports_are_declared_everywhere(pkg, lib):
    hdr = open(os.path.join(ROOT, "include", "gmrf_hip.h")).read()
    shim = open(os.path.join(ROOT, "julia", "DiffEqGMRFsHIP.jl")).read()
    bound = _check_julia_ccalls(shim, hdr, 40)
    for name in NEW_EXPORTS:
        assert re.search(r"gmrf_status\s+%s\s*\(" % name, hdr), name
        assert name in pkg._cabi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
        assert name in bound, name
    assert "EllipticP1Tangent" in pkg.__all__
    for meth in ("tangent", "tangent_batch", "load"):
        assert hasattr(pkg.EllipticP1Tangent, meth)
    for fn in ("elliptic_gauss_newton", "elliptic_gauss_newton_batch", "solution_errors"):
        assert hasattr(pkg.workloads, fn)


@pytest.mark.parametrize("nx,ny", MESHES)
def test_pattern_only_handle_reports_the_darcy_pattern_and_the_oracles_qpoints(pkg, nx, ny):
    e = pkg.EllipticP1Tangent(nx, ny, device=-1)
    d = pkg.DarcyP1Assembler(nx, ny, device=-1)
    mesh = EO.Mesh(nx, ny)
    for ref in (d.pattern, mesh.pattern):
        assert np.array_equal(e.pattern.indptr, ref.indptr) and np.array_equal(e.pattern.indices, ref.indices)
    assert e.nnz == d.nnz and e.n == nx * ny and e.cells == len(mesh.cells)
    qo = EO.qpoints(mesh)
    assert e.qpoints.shape == qo.shape == (2 * (nx - 1) * (ny - 1), 3, 2)
    print(f"{nx}x{ny}: qpoints max |handle - oracle| {np.max(np.abs(e.qpoints - qo)):.2e}")
    assert np.max(np.abs(e.qpoints - qo)) <= 2.0 ** -52           # (coordinates in [0, 1]: one unit in the last place)
    assert np.max(np.abs(e.qpoints - pkg.workloads.p1_triangle_qpoints(nx, ny))) <= 2.0 ** -52
    assert np.array_equal(e.qpoints, pkg.ShallowWaterP1(nx, ny, device=-1).qpoints)


def test_calls_validate_their_arguments_without_a_gpu(pkg, lib):
    cabi = pkg._cabi
    nx, ny, B = 5, 4, 3
    e = pkg.EllipticP1Tangent(nx, ny, device=-1)
    W = np.zeros((B, e.n))
    for call in (lambda: e.tangent(W[0]), lambda: e.tangent_batch(W), lambda: e.load(np.zeros((e.cells, 3))),
                 lambda: e.load(np.zeros((B, e.cells, 3)))):
        with pytest.raises(pkg.GmrfError) as err:             # the numeric phase needs the GPU: no CPU fallback
            call()
        assert err.value.status == cabi.ERR_NO_DEVICE
    for call in (lambda: e.tangent(np.zeros(e.n + 1)), lambda: e.tangent_batch(np.zeros((B, e.n - 1))),
                 lambda: e.load(np.zeros((e.cells, 2))), lambda: e.load(np.zeros((B, e.cells + 1, 3)))):
        with pytest.raises(ValueError):
            call()
    P = cabi.ptr
    v, f, s = np.zeros((B, e.nnz)), np.zeros((B, e.n)), np.zeros((B, e.cells, 3))
    h = C.c_void_p()
    bad = [lib.gmrf_elliptic_p1_create(-1, None, 1, 4, C.byref(h)),
           lib.gmrf_elliptic_p1_create(-1, None, 4, 40000, C.byref(h)),
           lib.gmrf_elliptic_p1_create(-1, None, 4, 4, None),
           lib.gmrf_elliptic_p1_pattern(None, None, None, None, 0),
           lib.gmrf_elliptic_p1_qpoints(e._h, None),
           lib.gmrf_elliptic_p1_tangent(e._h, None, P(v), P(f)),
           lib.gmrf_elliptic_p1_tangent(None, P(W), P(v), P(f)),
           lib.gmrf_elliptic_p1_tangent_batch(e._h, 0, P(W), P(v), P(f)),
           lib.gmrf_elliptic_p1_tangent_batch(e._h, 4097, P(W), P(v), P(f)),
           lib.gmrf_elliptic_p1_tangent_batch(e._h, B, P(W), None, P(f)),
           lib.gmrf_elliptic_p1_load(e._h, 0, P(s), P(f)),
           lib.gmrf_elliptic_p1_load(e._h, 4097, P(s), P(f)),
           lib.gmrf_elliptic_p1_load(e._h, B, None, P(f)),
           lib.gmrf_elliptic_p1_load(None, B, P(s), P(f)),
           lib.gmrf_gn_create_elliptic(None, None, e._h, C.byref(h)),
           lib.gmrf_gn_create_elliptic(None, None, None, C.byref(h))]
    assert bad == [cabi.ERR_BAD_SHAPE] * len(bad), bad
    assert lib.gmrf_elliptic_p1_destroy(None) == cabi.GMRF_OK
    with pytest.raises(TypeError):
        pkg.GaussNewtonBatch(None, None, object())


def test_workload_holds_the_ingredients_of_the_reference_loop(pkg):
    wl = pkg.workloads
    w = wl.elliptic_gauss_newton_batch((19, 14), 4, amps=EO.GN_CASE["amps"])
    assert w["n_blocks"] == 7 and w["n"] == w["m"] == 266 and w["Q"].shape == (266, 266)
    assert wl.block_bandwidth_ok(w["Q"], w["n_blocks"])
    assert not np.any(w["x_prior"]) and not np.any(w["Qx_prior"]) and np.array_equal(w["x0"], w["x_prior"])
    # the truth vanishes on the boundary (to rounding) and solves the PDE: f_src = -Lap u + u^3 by central differences
    ix, iy = np.arange(266) % 19, np.arange(266) // 19
    bnd = (ix == 0) | (iy == 0) | (ix == 18) | (iy == 13)
    assert np.max(np.abs(w["truth"][:, bnd])) < 1e-15 * 4
    h = 1e-4
    for amp in (0.0, 2.0):
        x, y = np.array([0.3, 0.62]), np.array([0.41, 0.87])
        u, src = wl.elliptic_truth(x, y, amp)
        lap = (wl.elliptic_truth(x + h, y, amp)[0] + wl.elliptic_truth(x - h, y, amp)[0] + wl.elliptic_truth(x, y + h, amp)[0]
               + wl.elliptic_truth(x, y - h, amp)[0] - 4 * u) / h ** 2
        assert np.allclose(src, -lap + u ** 3, rtol=1e-5)
    one = wl.elliptic_gauss_newton((19, 14), amp=1.0)
    assert np.array_equal(one["src_q"], w["src_q"][2]) and np.array_equal(one["truth"], w["truth"][2])
    assert np.array_equal(one["Q"].data, w["q_values"]) and one["x0"].shape == (266,)
    # metrics of src/metrics.jl:3-13
    m = wl.solution_errors(np.array([1.0, 2.0, 5.0]), np.array([1.0, 4.0, 4.0]))
    assert m == {"rmse": pytest.approx(np.sqrt(5 / 3)), "max_err": 2.0, "rel_err": pytest.approx(np.sqrt(5 / 33))}


def test_oracle_cube_tangent_is_the_derivative_of_the_cubic_residual():
    mesh = EO.Mesh(7, 6)
    rng = np.random.default_rng(3)
    w = np.sin(np.pi * mesh.coords[:, 0]) * np.sin(np.pi * mesh.coords[:, 1]) + 0.1 * rng.standard_normal(mesh.n)
    vals, v = EO.assemble_J_cube(mesh, w)
    Jc = mesh.matrix(vals).toarray()
    h = 1e-6
    fd = np.empty((mesh.n, mesh.n))
    for j in range(mesh.n):
        e = np.zeros(mesh.n); e[j] = h
        fd[:, j] = (EO.assemble_J_cube(mesh, w + e)[1] - EO.assemble_J_cube(mesh, w - e)[1]) / (2 * h)
    # central differences of a cubic: the error is the third derivative's term, 6 int phi^4 h^2 ~ 1e-12, plus rounding / h
    print("max |J_cube - fd|", np.max(np.abs(Jc - fd)), "max |J_cube|", np.max(np.abs(Jc)))
    assert np.max(np.abs(Jc - fd)) < 1e-9
    assert np.max(np.abs(Jc)) > 1e-3


def test_oracle_prescribed_rows_are_zero_and_interior_rows_are_the_stiffness(pkg):
    for nx, ny in MESHES:
        mesh = EO.Mesh(nx, ny)
        rng = np.random.default_rng(nx)
        src = rng.standard_normal((len(mesh.cells), 3))
        w = rng.standard_normal(mesh.n)
        sv, fs = EO.assemble_J_diff_and_f(mesh, src)
        cv, v = EO.assemble_J_cube(mesh, w)
        f, J = EO.f_and_J(w, mesh, sv, fs)
        pres = sorted(mesh.prescribed)
        interior = sorted(set(range(mesh.n)) - mesh.prescribed)
        assert len(interior) == (nx - 2) * (ny - 2)
        for M in (mesh.matrix(sv), mesh.matrix(cv), J):
            assert not np.any(M.toarray()[pres])
        assert not np.any(fs[pres]) and not np.any(v[pres]) and not np.any(f[pres])
        G = pkg.workloads.p1_unit_square(nx, ny)[1].toarray()
        S = mesh.matrix(sv).toarray()
        assert np.max(np.abs(S[interior] - G[interior])) < 1e-13 * np.max(np.abs(G))
        assert np.any(S[interior][:, pres])                       # columns of prescribed dofs are kept
        # the load of a constant source is the lumped mass
        _, f1 = EO.assemble_J_diff_and_f(mesh, np.ones((len(mesh.cells), 3)))
        lumped = pkg.workloads.p1_unit_square(nx, ny)[0]
        assert np.allclose(f1[interior], lumped[interior], rtol=1e-13, atol=0)


def test_lock_step_oracle_reproduces_the_per_problem_loop(gn_cases):
    c = EO.GN_CASE
    w, prob, (x, steps, hist, rels, its) = gn_cases[(19, 14)]
    assert len(its) == steps.max()
    for p in (0, 3):
        xs, ss, hs, iters = EO.single_loop(prob.fJ(p), w["Q"], w["Qx_prior"][p], w["x_prior"][p], w["x0"][p], w["noise"], w["n_blocks"],
                                           c["rtol"], c["max_steps"])
        assert ss == steps[p] and np.array_equal(xs, x[p])
        assert np.array_equal(hs, hist[p, :ss + 1]) and np.all(np.isnan(hist[p, ss + 1:]))
        for it in range(len(its)):                                  # frozen after its last step
            assert np.array_equal(its[it][p], iters[min(it, ss - 1)])


@pytest.mark.parametrize("mesh_size", EO.GN_CASE["meshes"])
def test_gpu_case_is_well_conditioned_for_the_stop_rule(pkg, gn_cases, mesh_size):
    """The inputs of the GPU comparison (EO.GN_CASE), judged with the oracle alone: no tested ratio |last - cur| / |cur| lies
    within a factor 2 of rtol, so rounding cannot flip a stop decision; the problems stop at different counts (the freeze path
    runs) and before max_steps; every continuing ratio is far above the threshold; the iterates approach the truth."""
    c = EO.GN_CASE
    w, prob, (x, steps, hist, rels, its) = gn_cases[mesh_size]
    margin = GO.stop_margin(rels, c["rtol"])
    print(mesh_size, "steps", steps, "margin", margin)
    assert margin > 2.0
    assert steps.tolist() == [4, 4, 5, 5]
    assert len(set(steps.tolist())) >= 2 and steps.max() < c["max_steps"]
    for p in range(c["B"]):
        cont = rels[p, :steps[p]]                                   # the ratios after which the problem went on
        assert np.all(cont >= 1.3e-4)
        err = pkg.workloads.solution_errors(x[p], w["truth"][p])
        assert err["rel_err"] < 0.02 and err["max_err"] < 0.05 and err["rmse"] <= err["max_err"]
