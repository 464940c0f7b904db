"""The quadratic-triangle elliptic tangent and its Gauss-Newton workload: what can be checked without a GPU (the pattern-only
handle, the NumPy oracle's own consistency, the workload's partition rule and the conditioning of the GPU test's inputs)."""
import os
import re

import numpy as np
import pytest

from oracle import bt_oracle as O
from tests import elliptic_p2_oracle as PO
from tests import gn_batch_oracle as GO
from tests.test_host_logic import _check_julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESHES = ((2, 2), (3, 3), (8, 8), (10, 8))


@pytest.fixture(scope="module")
def gn_cases(pkg):
    """PO.GN_CASE_P2 on both meshes, computed once: mesh -> (workload, Problem, batch_loop result)."""
    return {ms: PO.oracle_case(pkg.workloads, ms) for ms in PO.GN_CASE_P2["meshes"]}


def _unit_coefficient_stiffness(nx, ny):
    g = np.linspace(0.0, 1.0, 3)
    return O.assemble_darcy_diff_matrix_p2(nx, ny, g, g, np.ones((3, 3)), constrain=False)[0]


def test_new_export_is_declared_everywhere(pkg, lib):
    name = "gmrf_elliptic_p2_create"
    hdr = open(os.path.join(ROOT, "include", "gmrf_hip.h")).read()
    shim = open(os.path.join(ROOT, "julia", "DiffEqGMRFsHIP.jl")).read()
    assert re.search(r"gmrf_status\s+%s\s*\(" % name, hdr)
    assert name in pkg._cabi.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert name in _check_julia_ccalls(shim, hdr, 40)
    for fn in ("p2_unit_square", "p2_triangle_qpoints"):
        assert hasattr(pkg.workloads, fn)


@pytest.mark.parametrize("nx,ny", MESHES)
def test_pattern_only_handle_reports_the_darcy_p2_pattern_and_the_oracles_qpoints(pkg, nx, ny):
    e = pkg.EllipticP1Tangent(nx, ny, device=-1, order=2)
    d = pkg.DarcyP1Assembler(nx, ny, device=-1, order=2)
    mesh = PO.Mesh(nx, ny)
    for ref in (d.pattern, mesh.pattern):
        assert np.array_equal(e.pattern.indptr, ref.indptr) and np.array_equal(e.pattern.indices, ref.indices)
    assert e.order == 2 and e.nq == 4 and e.nnz == d.nnz
    assert e.n == e.rows == (2 * nx - 1) * (2 * ny - 1) and e.cells == len(mesh.cells) == 2 * (nx - 1) * (ny - 1)
    qo = PO.qpoints(mesh)
    assert e.qpoints.shape == qo.shape == (e.cells, 4, 2)
    assert np.array_equal(e.qpoints, qo)                           # bit for bit: the unfused expression on both sides
    assert np.array_equal(e.qpoints, pkg.workloads.p2_triangle_qpoints(nx, ny))
    # every point lies strictly inside its cell's bounding box
    assert np.all(e.qpoints[:, :, 0] > mesh.vx.min(axis=1)[:, None]) and np.all(e.qpoints[:, :, 0] < mesh.vx.max(axis=1)[:, None])
    assert np.all(e.qpoints[:, :, 1] > mesh.vy.min(axis=1)[:, None]) and np.all(e.qpoints[:, :, 1] < mesh.vy.max(axis=1)[:, None])


def test_order_argument_and_shapes_without_a_gpu(pkg):
    with pytest.raises(ValueError):
        pkg.EllipticP1Tangent(4, 4, device=-1, order=3)
    with pytest.raises(ValueError):
        pkg.EllipticP1Tangent(4, 4, device=-1, order=0)
    with pytest.raises(ValueError):
        pkg.workloads.elliptic_gauss_newton_batch((8, 8), 1, rows_per_block=5, order=3)
    e1, e1d = pkg.EllipticP1Tangent(5, 4, device=-1), pkg.EllipticP1Tangent(5, 4, device=-1, order=1)
    assert e1.nq == e1d.nq == 3 and e1.n == e1d.n == 20 and e1d.order == 1
    assert np.array_equal(e1.pattern.indices, e1d.pattern.indices) and np.array_equal(e1.qpoints, e1d.qpoints)
    e = pkg.EllipticP1Tangent(5, 4, device=-1, order=2)
    for call in (lambda: e.tangent(np.zeros(e.n)), lambda: e.tangent_batch(np.zeros((2, e.n))), lambda: e.load(np.zeros((e.cells, 4))),
                 lambda: e.load(np.zeros((2, e.cells, 4)))):
        with pytest.raises(pkg.GmrfError) as err:                 # the numeric phase needs the GPU: no CPU fallback
            call()
        assert err.value.status == pkg._cabi.ERR_NO_DEVICE
    for call in (lambda: e.tangent(np.zeros(20)), lambda: e.tangent_batch(np.zeros((2, 20))), lambda: e.load(np.zeros((e.cells, 3))),
                 lambda: e.load(np.zeros((2, e.cells, 3)))):
        with pytest.raises(ValueError):
            call()


@pytest.mark.parametrize("nx,ny", MESHES)
def test_oracle_static_values_are_the_darcy_p2_stiffness_with_unit_coefficient(nx, ny):
    mesh = PO.Mesh(nx, ny)
    G = _unit_coefficient_stiffness(nx, ny)
    assert np.array_equal(G.indptr, mesh.pattern.indptr) and np.array_equal(G.indices, mesh.pattern.indices)
    sv, _ = PO.assemble_J_diff_and_f(mesh, np.zeros((len(mesh.cells), 4)), mask_rows=False)
    err = np.max(np.abs(sv - G.data))
    print(f"{nx}x{ny}: max |static - G| {err:.2e}, max |G| {np.max(np.abs(G.data)):.3e}")
    assert err <= 1e-14 * np.max(np.abs(G.data))
    # masked: prescribed rows zero, interior rows untouched, prescribed columns kept
    mv, _ = PO.assemble_J_diff_and_f(mesh, np.zeros((len(mesh.cells), 4)))
    S, Sm = mesh.matrix(sv).toarray(), mesh.matrix(mv).toarray()
    pres = sorted(mesh.prescribed)
    interior = sorted(set(range(mesh.n)) - mesh.prescribed)
    assert len(interior) == (2 * nx - 3) * (2 * ny - 3)
    assert not np.any(Sm[pres]) and np.array_equal(Sm[interior], S[interior]) and np.any(Sm[interior][:, pres])


def test_oracle_tangent_is_the_derivative_of_the_residual():
    """J(w) d against the central difference of f along a random d.  The rule integrates J and f with the same points, so J is
    the exact derivative of the discrete f: what is left is the difference's own error, h^2 |f'''| / 6 ~ 1e-10 relative with
    h = 1e-5, plus rounding / h ~ 1e-11."""
    mesh = PO.Mesh(5, 4)
    rng = np.random.default_rng(3)
    w = np.sin(np.pi * mesh.coords[:, 0]) * np.sin(np.pi * mesh.coords[:, 1]) + 0.1 * rng.standard_normal(mesh.n)
    d = rng.standard_normal(mesh.n)
    sv, fs = PO.assemble_J_diff_and_f(mesh, rng.standard_normal((len(mesh.cells), 4)))
    _, J = PO.f_and_J(w, mesh, sv, fs)
    h = 1e-5
    fd = (PO.f_and_J(w + h * d, mesh, sv, fs)[0] - PO.f_and_J(w - h * d, mesh, sv, fs)[0]) / (2 * h)
    err = np.linalg.norm(J @ d - fd) / np.linalg.norm(fd)
    print("rel |J d - fd|", err)
    assert err < 1e-6
    cube = mesh.matrix(PO.assemble_J_cube(mesh, w)[0])
    assert np.linalg.norm(cube @ d) > 1e-3 * np.linalg.norm(J @ d)          # (the cubic part takes part in the comparison)


def test_oracle_load_of_a_constant_source_is_the_consistent_mass_row_sum():
    """int N_i over the mesh: |T| / 3 per cell for an edge midpoint and 0 for a vertex -- why row-sum lumping is unusable."""
    mesh = PO.Mesh(4, 3)
    _, f1 = PO.assemble_J_diff_and_f(mesh, np.ones((len(mesh.cells), 4)), mask_rows=False)
    I, J = np.arange(mesh.n) % mesh.W, np.arange(mesh.n) // mesh.W
    vertex = (I % 2 == 0) & (J % 2 == 0)
    assert np.max(np.abs(f1[vertex])) < 1e-15 and np.all(f1[~vertex] > 1e-3)
    assert abs(f1.sum() - 1.0) < 1e-14


@pytest.mark.parametrize("nx,ny", ((8, 8), (10, 8)))
def test_p2_unit_square_is_the_oracles_stiffness_with_a_positive_lumped_mass(pkg, nx, ny):
    lumped, G, (X, Y) = pkg.workloads.p2_unit_square(nx, ny)
    Go = _unit_coefficient_stiffness(nx, ny)
    assert np.array_equal(G.indptr, Go.indptr) and np.array_equal(G.indices, Go.indices)
    assert np.max(np.abs(G.data - Go.data)) <= 1e-14 * np.max(np.abs(Go.data))
    assert np.all(lumped > 0.0) and abs(lumped.sum() - 1.0) < 1e-14
    mesh = PO.Mesh(nx, ny)
    assert np.array_equal(np.stack([X, Y], axis=1), mesh.coords)
    assert X.min() == 0.0 and X.max() == 1.0 and Y.min() == 0.0 and Y.max() == 1.0
    # HRZ: one cell gives |T| / 19 to a vertex and 16 |T| / 57 to a midpoint; a corner vertex of the mesh has one or two cells
    area = 0.5 / ((nx - 1) * (ny - 1))
    assert lumped[0] == pytest.approx(2 * area / 19.0, rel=1e-14)            # (0, 0): the lower and the upper cell of its quad
    assert lumped[1] == pytest.approx(16 * area / 57.0, rel=1e-14)           # a boundary edge midpoint: one cell


def test_workload_partition_rule_and_ingredients(pkg):
    wl = pkg.workloads
    for ms in PO.GN_CASE_P2["meshes"]:
        w = wl.elliptic_gauss_newton_batch(ms, 4, rows_per_block=5, amps=PO.GN_CASE_P2["amps"], order=2)
        W, H = 2 * ms[0] - 1, 2 * ms[1] - 1
        assert w["n"] == w["m"] == W * H and w["n_blocks"] == H // 5 == 3 and w["Q"].shape == (W * H, W * H)
        assert w["qpoints"].shape == (w["src_q"].shape[1], 4, 2) and w["src_q"].shape[0] == 4 and w["truth"].shape == (4, W * H)
        assert wl.block_bandwidth_ok(w["Q"], w["n_blocks"])
        assert not np.any(w["x_prior"]) and not np.any(w["Qx_prior"]) and np.array_equal(w["x0"], w["x_prior"])
        I, J = np.arange(W * H) % W, np.arange(W * H) // W
        bnd = (I == 0) | (J == 0) | (I == W - 1) | (J == H - 1)
        assert np.max(np.abs(w["truth"][:, bnd])) < 1e-15 * 4
        assert np.all(w["Q"].diagonal()[bnd] > 1e11)                        # bnd_noise on the boundary lattice points
        with pytest.raises(AssertionError):                                 # reach 4 rows: 3 rows per block are too few
            wl.elliptic_gauss_newton_batch(ms, 1, rows_per_block=3, order=2)
    with pytest.raises(AssertionError):                                     # 2 ny - 1 = 17 is no multiple of 5
        wl.elliptic_gauss_newton_batch((8, 9), 1, rows_per_block=5, order=2)
    one = wl.elliptic_gauss_newton((10, 8), rows_per_block=5, amp=1.0, order=2)
    w = wl.elliptic_gauss_newton_batch((10, 8), 4, rows_per_block=5, amps=PO.GN_CASE_P2["amps"], order=2)
    assert np.array_equal(one["src_q"], w["src_q"][2]) and np.array_equal(one["truth"], w["truth"][2])
    assert np.array_equal(one["Q"].data, w["q_values"]) and one["x0"].shape == (285,)


def test_order_1_is_the_call_without_the_argument(pkg):
    wl = pkg.workloads
    for a, b in ((wl.elliptic_gauss_newton_batch((19, 14), 3), wl.elliptic_gauss_newton_batch((19, 14), 3, order=1)),
                 (wl.elliptic_gauss_newton(16, amp=0.5), wl.elliptic_gauss_newton(16, amp=0.5, order=1))):
        assert a.keys() == b.keys()
        for k in a:
            if k == "Q":
                assert np.array_equal(a[k].indptr, b[k].indptr) and np.array_equal(a[k].indices, b[k].indices)
                assert np.array_equal(a[k].data, b[k].data)
            else:
                assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize("mesh_size", PO.GN_CASE_P2["meshes"])
def test_gpu_case_is_well_conditioned_for_the_stop_rule(pkg, gn_cases, mesh_size):
    """The inputs of the GPU comparison (PO.GN_CASE_P2), judged with the oracle alone (through O.gn_step): no tested ratio
    |last - cur| / |cur| lies within a factor 5 of rtol, so rounding cannot flip a stop decision; the problems stop at at least two
    different counts (the freeze path runs) and before max_steps; the iterates approach the truth."""
    c = PO.GN_CASE_P2
    w, prob, (x, steps, hist, rels, its) = gn_cases[mesh_size]
    margin = GO.stop_margin(rels, c["rtol"])
    print(mesh_size, "steps", steps, "margin", margin)
    assert margin > 5.0
    assert len(set(steps.tolist())) >= 2 and steps.max() < c["max_steps"]
    assert len(its) == steps.max()
    for p in range(c["B"]):
        err = pkg.workloads.solution_errors(x[p], w["truth"][p])
        print(p, err)
        assert err["rel_err"] < 0.01 and err["rmse"] <= err["max_err"]
    # the lock-step oracle reproduces the per-problem loop
    p = int(np.argmin(steps))
    xs, ss, hs, _ = PO.single_loop(prob.fJ(p), w["Q"], w["Qx_prior"][p], w["x_prior"][p], w["x0"][p], w["noise"], w["n_blocks"],
                                   c["rtol"], c["max_steps"])
    assert ss == steps[p] and np.array_equal(xs, x[p]) and np.array_equal(hs, hist[p, :ss + 1])
