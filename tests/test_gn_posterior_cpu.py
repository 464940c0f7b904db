"""The posterior stage of the batched Gauss-Newton loops: what can be checked without a GPU (the oracle of
tests/gn_posterior_oracle.py against an independent route, declarations, the package surface, argument validation of
gmrf_gn_posterior and its two building blocks)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.stats

from tests import gn_posterior_oracle as PO
from tests.test_host_logic import _check_julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["gmrf_bt_logdet_batch", "gmrf_assemble_quadform_batch", "gmrf_gn_posterior"]


@pytest.mark.parametrize("n_blocks,bs,seed", [(4, 12, 0), (3, 16, 5), (6, 7, 9)])
def test_oracle_against_scipy_multivariate_normal(pkg, n_blocks, bs, seed):
    """-logpdf of N(x, A^-1) at z from scipy.stats (dense inverse, its own eigendecomposition) equals the oracle's nll to 1e-10
    relative on well conditioned matrices of n <= 48; sqmahal against the dense float64 form at its own rounding level."""
    w = pkg.workloads.random_block_tridiagonal(n_blocks, bs, seed=seed)
    A, n = w.Q, w.n
    assert n <= 48 and np.linalg.cond(A.toarray()) < 1e3
    rng = np.random.default_rng(seed + 1)
    x, z = rng.standard_normal(n), rng.standard_normal(n)
    got = float(PO.nll(A, x, z))
    ref = -scipy.stats.multivariate_normal(mean=x, cov=np.linalg.inv(A.toarray())).logpdf(z)
    print(f"n={n}: oracle nll {got:.15e} scipy {ref:.15e} rel {abs(got - ref) / abs(ref):.2e}")
    assert abs(got - ref) <= 1e-10 * abs(ref)
    d = z - x
    dense = float(d @ (A.toarray() @ d))
    assert abs(float(PO.sqmahal(A, x, z)) - dense) <= (n + 2) * PO.EPS * float(PO.abs_form(A, x, z))
    assert abs(float(PO.logdet_ld(A)) - np.linalg.slogdet(A.toarray())[1]) <= 1e-12 * abs(np.linalg.slogdet(A.toarray())[1])


def test_bound_counts_the_kernels_operations():
    """depth = 2 + cmax + run + 8 + nch + 8 on the shape of the device test (ns = 72, nt = 30: two chunks of 1080 columns, a
    thread's run of 5 that ends mid-stride) and on one chunk; the bound notices a relative error of 2^-40
    and a dropped column."""
    assert PO.chunks(2160) == (2, 1080) and PO.chunks(512) == (1, 512) and PO.chunks(2048 * 1024 + 5) == (1024, 2049)
    n = 2160
    A = (sp.diags([np.full(n - 1, -1.0), np.full(n, 4.0), np.full(n - 1, -1.0)], [-1, 0, 1]) +
         sp.csr_matrix(([-1.0, -1.0], ([0, n - 1], [n - 1, 0])), shape=(n, n))).tocsc()
    assert PO.depth(A) == 2 + 3 + 5 + 8 + 2 + 8
    rng = np.random.default_rng(3)
    x, z = rng.standard_normal(n), rng.standard_normal(n)
    exact, bound = PO.sqmahal(A, x, z), PO.quadform_bound(A, x, z)
    d = z - x
    f64 = float(d @ (A @ d))
    assert abs(f64 - float(exact)) <= bound                               # a float64 evaluation of another order: inside
    assert bound < 1e-13 * float(exact)
    j = 1000
    assert abs(float(exact)) * 2.0 ** -40 > bound                         # every term off by a relative 2^-40: outside
    assert abs(float(d[j] * (A[:, [j]].T @ d)[0])) > bound                # column j dropped: outside


def test_new_exports_are_declared_everywhere(pkg, lib):
    hdr = open(os.path.join(ROOT, "include", "gmrf_hip.h")).read()
    shim = open(os.path.join(ROOT, "julia", "DiffEqGMRFsHIP.jl")).read()
    bound = _check_julia_ccalls(shim, hdr, 40)
    for name in NEW_EXPORTS:
        assert re.search(r"gmrf_status\s+%s\s*\(" % name, hdr), name
        assert name in pkg._cabi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
        assert name in bound, name
    # the three descriptions of gmrf_gn_posterior agree: 16 arguments, the same kinds in the same order
    proto = re.search(r"gmrf_status\s+gmrf_gn_posterior\s*\(([^;]*?)\);", hdr, flags=re.S).group(1)
    kinds = ["ptr" if "*" in a else a.split()[0] for a in proto.split(",")]
    ctypes_kind = {C.c_void_p: "ptr", C.POINTER(C.c_int32): "ptr", C.c_int64: "int64_t", C.c_int32: "int32_t", C.c_uint64: "uint64_t"}
    assert kinds == [ctypes_kind[t] for t in lib.gmrf_gn_posterior.argtypes] and len(kinds) == 16
    for fn in ("function logdet_batch", "function quadform_batch!", "function posterior!"):
        assert fn in shim, fn
    assert hasattr(pkg, "GaussNewtonPosterior") and "GaussNewtonPosterior" in pkg.__all__
    assert hasattr(pkg.GaussNewtonBatch, "posterior") and hasattr(pkg.TridiagonalCholeskyFactor, "logdet_batch")
    assert hasattr(pkg.PosteriorAssembler, "quadform_batch")
    r = pkg.GaussNewtonPosterior()
    assert all(getattr(r, f) is None for f in ("x", "samples", "std", "std_norm", "logdet", "sqmahal", "nll", "errors"))


def test_posterior_refuses_bad_arguments_without_a_gpu(pkg, lib):
    """gmrf_gn_posterior: a null driver, then everything that is decided before the driver is looked at, with a driver pointer
    that is never followed; the building blocks' null pointers and pattern-only handles."""
    cabi = pkg._cabi
    P = cabi.ptr
    B, n = 2, 5
    z, buf = np.zeros((B, n)), np.full((B, 3, n), 7.0)
    info = C.c_int32(5)

    def post(g, zz=None, first=0, ks=1, method=cabi.VAR_RBMC, kv=50, samples=None, std=None, norm=None, ld=None, sq=None, nl=None,
             err=None):
        return lib.gmrf_gn_posterior(g, zz, first, ks, 1, method, kv, 1, samples, std, norm, ld, sq, nl, err, C.byref(info))

    assert post(None) == cabi.ERR_BAD_SHAPE
    fake = C.c_void_p(1)                    # (never dereferenced: each call below fails on an argument checked first)
    o = P(buf)
    bad = [post(fake, ks=-1), post(fake, ks=129),                                              # k_samples outside [0, 128]
           post(fake, method=3), post(fake, method=-2),                                        # an unknown var_method
           post(fake, method=cabi.VAR_RBMC, kv=0), post(fake, method=cabi.VAR_MC, kv=-4),      # k_var <= 0 with a sampled method
           post(fake, method=-1, std=o), post(fake, method=-1, norm=o),                        # std outputs without a method
           post(fake, ks=0, samples=o),                                                        # samples_out with k_samples = 0
           post(fake, sq=o), post(fake, nl=o), post(fake, err=o),                              # a score output with z = NULL
           post(fake, zz=P(z), first=-1, err=o)]
    assert bad == [cabi.ERR_BAD_SHAPE] * len(bad), bad
    assert info.value == 0 and np.all(buf == 7.0)
    # the building blocks
    out = np.full(B, 7.0)
    assert lib.gmrf_bt_logdet_batch(None, P(out)) == cabi.ERR_BAD_SHAPE
    Q = sp.identity(n, format="csc") * 2.0
    J = sp.csr_matrix(np.eye(3, n))
    asm = pkg.PosteriorAssembler(Q, J, device=-1)
    a = np.ones((B, asm.nnz_out))
    bad = [lib.gmrf_assemble_quadform_batch(None, B, P(a), asm.nnz_out, P(z), P(z), P(out)),
           lib.gmrf_assemble_quadform_batch(asm._h, 0, P(a), asm.nnz_out, P(z), P(z), P(out)),
           lib.gmrf_assemble_quadform_batch(asm._h, 4097, P(a), asm.nnz_out, P(z), P(z), P(out)),
           lib.gmrf_assemble_quadform_batch(asm._h, B, None, asm.nnz_out, P(z), P(z), P(out)),
           lib.gmrf_assemble_quadform_batch(asm._h, B, P(a), asm.nnz_out, None, P(z), P(out)),
           lib.gmrf_assemble_quadform_batch(asm._h, B, P(a), asm.nnz_out, P(z), None, P(out)),
           lib.gmrf_assemble_quadform_batch(asm._h, B, P(a), asm.nnz_out, P(z), P(z), None),
           lib.gmrf_assemble_quadform_batch(asm._h, B, P(a), asm.nnz_out - 1, P(z), P(z), P(out))]
    assert bad == [cabi.ERR_BAD_SHAPE] * len(bad), bad
    # the numeric phase needs the GPU: no CPU fallback
    with pytest.raises(pkg.GmrfError) as e:
        asm.quadform_batch(a, z, z)
    assert e.value.status == cabi.ERR_NO_DEVICE
    with pytest.raises(ValueError):
        asm.quadform_batch(a[:, :-1], z, z)
    assert np.all(out == 7.0)
