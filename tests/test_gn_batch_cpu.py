"""Batched Gauss-Newton for the Burgers data-set loop: what can be checked without a GPU (declarations, argument validation,
the batch workload, the NumPy oracle of the lock-step loop and the conditioning of the GPU test's inputs)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import gn_batch_oracle as GO
from tests.test_host_logic import _check_julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["gmrf_burgers_p1_tangent_batch", "gmrf_assemble_precision_batch", "gmrf_assemble_rhs_batch",
               "gmrf_assemble_objective_batch", "gmrf_gn_create", "gmrf_gn_destroy", "gmrf_gn_run", "gmrf_gn_finalize"]


def test_new_exports_are_declared_everywhere(pkg, lib):
    hdr = open(os.path.join(ROOT, "include", "gmrf_hip.h")).read()
    shim = open(os.path.join(ROOT, "julia", "DiffEqGMRFsHIP.jl")).read()
    bound = _check_julia_ccalls(shim, hdr, 40)
    for name in NEW_EXPORTS:
        assert re.search(r"gmrf_status\s+%s\s*\(" % name, hdr), name
        assert name in pkg._cabi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
        assert name in bound, name
    assert "function gauss_newton_batch!" in shim
    for cls in ("GaussNewtonBatch",):
        assert hasattr(pkg, cls)
    for meth in ("precision_batch", "rhs_batch", "objective_batch"):
        assert hasattr(pkg.PosteriorAssembler, meth)
    assert hasattr(pkg.BurgersP1Tangent, "tangent_batch")


def test_batch_building_blocks_validate_their_arguments_without_a_gpu(pkg, lib):
    ns, nt, B = 16, 5, 3
    cabi = pkg._cabi
    b = pkg.BurgersP1Tangent(ns, nt, 0.25, 0.01, device=-1)
    g = pkg.workloads.burgers_gauss_newton(ns, nt)
    asm = pkg.PosteriorAssembler(g["Q"], b.pattern, device=-1)
    W = np.zeros((B, b.n))
    # the numeric phase needs the GPU: no CPU fallback
    for call in (lambda: b.tangent_batch(W),
                 lambda: asm.precision_batch(g["Q"].data, np.zeros((B, asm.nnz_j)), 1.0),
                 lambda: asm.rhs_batch(None, np.zeros((B, asm.nnz_j)), W, None, 1.0),
                 lambda: asm.objective_batch(g["Q"].data, W, W, np.zeros((B, asm.m)), 1.0)):
        with pytest.raises(pkg.GmrfError) as e:
            call()
        assert e.value.status == cabi.ERR_NO_DEVICE
    # shapes are checked before anything is sent to the library
    with pytest.raises(ValueError):
        b.tangent_batch(np.zeros((B, b.n + 1)))
    with pytest.raises(ValueError):
        asm.precision_batch(np.zeros((B, asm.nnz_q + 1)), np.zeros((B, asm.nnz_j)), 1.0)
    with pytest.raises(ValueError):
        asm.rhs_batch(None, np.zeros((B, asm.nnz_j)), np.zeros((B + 1, asm.n)), None, 1.0)
    with pytest.raises(ValueError):
        asm.objective_batch(g["Q"].data, W, W, np.zeros((B, asm.m - 1)), 1.0)
    # the C ABI itself: null pointers, batch outside [1, 4096], a q_stride that is neither 0 nor nnz(Q)
    v, f = np.zeros((B, b.nnz)), np.zeros((B, b.rows))
    q, out = np.zeros(asm.nnz_q), np.zeros((B, asm.nnz_out))
    P = cabi.ptr
    bad = [lib.gmrf_burgers_p1_tangent_batch(b._h, 0, P(W), P(v), P(f)),
           lib.gmrf_burgers_p1_tangent_batch(b._h, 4097, P(W), P(v), P(f)),
           lib.gmrf_burgers_p1_tangent_batch(b._h, B, None, P(v), P(f)),
           lib.gmrf_burgers_p1_tangent_batch(None, B, P(W), P(v), P(f)),
           lib.gmrf_assemble_precision_batch(asm._h, 0, P(q), 0, P(v), 1.0, P(out)),
           lib.gmrf_assemble_precision_batch(asm._h, B, P(q), 7, P(v), 1.0, P(out)),
           lib.gmrf_assemble_precision_batch(asm._h, B, None, 0, P(v), 1.0, P(out)),
           lib.gmrf_assemble_precision_batch(None, B, P(q), 0, P(v), 1.0, P(out)),
           lib.gmrf_assemble_rhs_batch(asm._h, -1, None, P(v), P(W), None, 1.0, P(W)),
           lib.gmrf_assemble_rhs_batch(asm._h, B, None, None, P(W), None, 1.0, P(W)),
           lib.gmrf_assemble_objective_batch(asm._h, B, P(q), 3, P(W), P(W), P(f), 1.0, P(np.zeros(B))),
           lib.gmrf_assemble_objective_batch(asm._h, B, P(q), 0, P(W), P(W), None, 1.0, P(np.zeros(B))),
           lib.gmrf_gn_create(None, asm._h, b._h, C.byref(C.c_void_p())),
           lib.gmrf_gn_run(None, P(q), 0, P(W), P(W), P(W), None, 1.0, 1e-4, 3, None, None, None),
           lib.gmrf_gn_finalize(None, None)]
    assert bad == [cabi.ERR_BAD_SHAPE] * len(bad), bad
    assert lib.gmrf_gn_destroy(None) == cabi.GMRF_OK


def test_batch_workload_is_deterministic_and_problem_0_is_the_single_workload(pkg):
    ns, nt, B = 64, 8, 4
    a = pkg.workloads.burgers_gauss_newton_batch(ns, nt, B, seed=0)
    c = pkg.workloads.burgers_gauss_newton_batch(ns, nt, B, seed=0)
    for k in ("q_values", "Qx_prior", "x_prior", "x0", "ic"):
        assert np.array_equal(a[k], c[k]), k
        assert a[k].shape[0] == B
    one = pkg.workloads.burgers_gauss_newton(ns, nt)
    assert np.array_equal(a["Q"].indptr, one["Q"].indptr) and np.array_equal(a["Q"].indices, one["Q"].indices)
    assert np.array_equal(a["q_values"][0], one["Q"].data)
    assert np.array_equal(a["Qx_prior"][0], one["Qx_prior"]) and np.array_equal(a["x_prior"][0], one["x_prior"])
    assert a["noise"] == one["noise"] and a["n_blocks"] == one["n_blocks"]
    # the problems differ: initial conditions, priors (through the bulk speed) and start points
    assert not np.array_equal(a["ic"][0], a["ic"][1]) and not np.array_equal(a["q_values"][0], a["q_values"][1])
    assert np.array_equal(a["x0"][:, :ns], a["ic"]) and np.array_equal(a["x0"][:, ns:], a["x_prior"][:, ns:])
    d = pkg.workloads.burgers_gauss_newton_batch(ns, nt, B, seed=1)
    assert np.array_equal(d["ic"][0], a["ic"][0]) and not np.array_equal(d["ic"][1], a["ic"][1])


def test_lock_step_oracle_reproduces_the_per_problem_loop(pkg):
    """32 x 6: the lock-step restatement (every problem solved in every iteration, frozen ones dropped) gives exactly what
    the reference's loop gives problem by problem."""
    ns, nt, B, rtol, max_steps = 32, 6, 4, 1e-4, 12
    w = pkg.workloads.burgers_gauss_newton_batch(ns, nt, B, seed=3)
    x, steps, hist, rels, its = GO.batch_loop(ns, nt, w["dt"], w["nu"], w["Q"], w["q_values"], w["Qx_prior"], w["x_prior"], w["x0"],
                                              w["noise"], nt, rtol, max_steps)
    assert len(its) == steps.max()
    for p in range(B):
        Q = GO.problem_matrix(w["Q"], w["q_values"][p])
        xs, ss, hs, iters = GO.single_loop(ns, nt, w["dt"], w["nu"], Q, w["Qx_prior"][p], w["x_prior"][p], w["x0"][p], w["noise"],
                                           nt, rtol, max_steps)
        assert ss == steps[p] and np.array_equal(xs, x[p])
        assert np.array_equal(hs, hist[p, :ss + 1]) and np.all(np.isnan(hist[p, ss + 1:]))
        for it in range(len(its)):                      # frozen after its last step
            assert np.array_equal(its[it][p], iters[min(it, ss - 1)])
    # a shared Q (one value array) is the same loop
    x1, s1, h1, _, _ = GO.batch_loop(ns, nt, w["dt"], w["nu"], w["Q"], w["q_values"][0], w["Qx_prior"][:1], w["x_prior"][:1],
                                     w["x0"][:1], w["noise"], nt, rtol, max_steps)
    assert np.array_equal(x1[0], x[0]) and s1[0] == steps[0]


def test_gpu_case_is_well_conditioned_for_the_stop_rule(pkg):
    """The inputs of the GPU comparison (GO.GN_CASE), judged with the oracle alone: no tested ratio |last - cur| / |cur| lies
    within a factor 2 of rtol, so rounding cannot flip a stop decision; the problems stop at different counts (the freeze
    path runs) and before max_steps."""
    c = GO.GN_CASE
    w = pkg.workloads.burgers_gauss_newton_batch(c["ns"], c["nt"], c["B"], seed=c["seed"])
    x, steps, hist, rels, its = GO.batch_loop(c["ns"], c["nt"], w["dt"], w["nu"], w["Q"], w["q_values"], w["Qx_prior"], w["x_prior"],
                                              w["x0"], w["noise"], c["nt"], c["rtol"], c["max_steps"])
    print("steps", steps, "margin", GO.stop_margin(rels, c["rtol"]))
    assert GO.stop_margin(rels, c["rtol"]) > 2.0
    assert len(set(steps.tolist())) >= 2 and steps.max() < c["max_steps"] and steps.min() >= 3
