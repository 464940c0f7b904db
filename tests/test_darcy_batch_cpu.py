"""Batched conditioning for the Darcy data-set loop: what can be checked without a GPU (declarations, the package surface,
argument validation of the new entry points)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.test_host_logic import _check_julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["gmrf_darcy_p1_assemble_batch", "gmrf_dc_create", "gmrf_dc_destroy", "gmrf_dc_run"]


def test_new_exports_are_declared_everywhere(pkg, lib):
    hdr = open(os.path.join(ROOT, "include", "gmrf_hip.h")).read()
    shim = open(os.path.join(ROOT, "julia", "DiffEqGMRFsHIP.jl")).read()
    bound = _check_julia_ccalls(shim, hdr, 40)
    for name in NEW_EXPORTS:
        assert re.search(r"gmrf_status\s+%s\s*\(" % name, hdr), name
        assert name in pkg._cabi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
        assert name in bound, name
    assert "typedef struct gmrf_dc gmrf_dc;" in hdr
    assert "function condition_on_observations_batch" in shim and "function assemble_batch!" in shim
    for cls in ("DarcyConditioningBatch", "DarcyConditioningResult"):
        assert hasattr(pkg, cls) and cls in pkg.__all__
    assert hasattr(pkg.DarcyP1Assembler, "assemble_batch") and hasattr(pkg.DarcyConditioningBatch, "run")
    assert hasattr(pkg.DarcyConditioningBatch, "close")


def test_batch_entry_points_validate_their_arguments_without_a_gpu(pkg, lib):
    nx, ny, ng, B = 6, 5, 7, 3
    cabi = pkg._cabi
    P = cabi.ptr
    for order in (1, 2):
        d = pkg.DarcyP1Assembler(nx, ny, device=-1, order=order)
        T = np.ones((B, ng, ng))
        # the numeric phase needs the GPU: no CPU fallback
        with pytest.raises(pkg.GmrfError) as e:
            d.assemble_batch(T)
        assert e.value.status == cabi.ERR_NO_DEVICE
        # shapes are checked before anything is sent to the library
        with pytest.raises(ValueError):
            d.assemble_batch(np.ones((B, ng, ng + 1)))
        with pytest.raises(ValueError):
            d.assemble_batch(np.ones((ng, ng)))
        v, f = np.zeros((B, d.nnz)), np.zeros((B, d.n))
        bad = [lib.gmrf_darcy_p1_assemble_batch(None, B, P(T), ng, 1.0, P(v), P(f)),
               lib.gmrf_darcy_p1_assemble_batch(d._h, 0, P(T), ng, 1.0, P(v), P(f)),
               lib.gmrf_darcy_p1_assemble_batch(d._h, -2, P(T), ng, 1.0, P(v), P(f)),
               lib.gmrf_darcy_p1_assemble_batch(d._h, 4097, P(T), ng, 1.0, P(v), P(f)),
               lib.gmrf_darcy_p1_assemble_batch(d._h, B, P(T), 0, 1.0, P(v), P(f)),
               lib.gmrf_darcy_p1_assemble_batch(d._h, B, P(T), -1, 1.0, P(v), P(f)),
               lib.gmrf_darcy_p1_assemble_batch(d._h, B, None, ng, 1.0, P(v), P(f)),
               lib.gmrf_darcy_p1_assemble_batch(d._h, B, P(T), ng, 1.0, None, P(f))]
        assert bad == [cabi.ERR_BAD_SHAPE] * len(bad), bad
        assert np.all(v == 0.0) and np.all(f == 0.0)


def test_driver_create_and_run_refuse_without_a_gpu(pkg, lib):
    import scipy.sparse as sp
    cabi = pkg._cabi
    P = cabi.ptr
    d = pkg.DarcyP1Assembler(6, 5, device=-1)
    Q0 = sp.identity(d.n, format="csc") * 2.0
    asm = pkg.PosteriorAssembler(Q0, d.pattern, device=-1)
    out = C.c_void_p()
    # like every other create: no device, no object
    assert lib.gmrf_dc_create(None, asm._h, d._h, C.byref(out)) == cabi.ERR_NO_DEVICE
    assert b"device" in lib.gmrf_last_error() and not out.value
    # null pointers
    assert lib.gmrf_dc_create(None, None, d._h, C.byref(out)) == cabi.ERR_BAD_SHAPE
    assert lib.gmrf_dc_create(None, asm._h, None, C.byref(out)) == cabi.ERR_BAD_SHAPE
    assert lib.gmrf_dc_create(None, asm._h, d._h, None) == cabi.ERR_BAD_SHAPE
    assert lib.gmrf_dc_destroy(None) == cabi.GMRF_OK
    # gmrf_dc_run: a null driver, then everything that is decided before the driver is looked at
    T, q = np.ones((1, 7, 7)), np.ones(asm.nnz_q)
    info = C.c_int32(5)
    run = lambda g, tab, ng, qv, ks, method, kv: lib.gmrf_dc_run(g, tab, ng, 1.0, qv, 0, None, 1e8, ks, 1, method, kv, 1,     # noqa: E731
                                                                None, None, None, None, C.byref(info))
    assert run(None, P(T), 7, P(q), 1, cabi.VAR_RBMC, 50) == cabi.ERR_BAD_SHAPE
    fake = C.c_void_p(1)                    # (never dereferenced: each call below fails on an argument checked first)
    bad = [run(fake, None, 7, P(q), 1, cabi.VAR_RBMC, 50),
           run(fake, P(T), 7, None, 1, cabi.VAR_RBMC, 50),
           run(fake, P(T), 0, P(q), 1, cabi.VAR_RBMC, 50),
           run(fake, P(T), -3, P(q), 1, cabi.VAR_RBMC, 50),
           run(fake, P(T), 7, P(q), -1, cabi.VAR_RBMC, 50),
           run(fake, P(T), 7, P(q), 129, cabi.VAR_RBMC, 50),
           run(fake, P(T), 7, P(q), 1, 3, 50),
           run(fake, P(T), 7, P(q), 1, -2, 50),
           run(fake, P(T), 7, P(q), 1, cabi.VAR_RBMC, 0),
           run(fake, P(T), 7, P(q), 1, cabi.VAR_MC, -4)]
    assert bad == [cabi.ERR_BAD_SHAPE] * len(bad), bad
    # the Python object: no GPU, no object
    with pytest.raises(pkg.GmrfError):
        pkg.DarcyConditioningBatch(type("F", (), {"_h": None})(), asm, d)
