"""Longdouble statements of the scores of the Gauss-Newton posterior stage (gmrf_assemble_quadform_batch, gmrf_gn_posterior):
    sqmahal = (z - x)' A (z - x),     nll = 0.5 (n log(2 pi) + sqmahal - logdet A)
(scripts/burgers/solve_burgers_gmrf-collocation.jl:208-215, :262-263) from a SciPy matrix, and the bounds the device's values are
held to.  Not a test module.

The bound of the quadratic form (u = 2^-53 the unit roundoff, eps = 2 u, g(k) = k u / (1 - k u) <= k eps for k u <= 1/2)
---------------------------------------------------------------------------------------------------------------------
quadform_part (csrc/gn_posterior.hpp) evaluates  sum_j d_j (sum_e a_e d_r(e))  with d = fl(z - x) and fused multiply-adds:
  * d_j = (z_j - x_j)(1 + t), |t| <= u, the same rounded value wherever it is used: every product a_e d_r d_j carries two such
    factors                                                                                                         2 roundings
  * the inner sum of column j is a chain of one fma per stored entry, cmax = the most entries in a column        cmax roundings
  * the outer fma adds column j's term to the thread's sum: thread t of a chunk of `len` columns takes the columns
    t, t + 256, ..., a chain of run = ceil(len / 256) fmas                                                         run roundings
  * block_sum_256 adds the workgroup's 256 sums in a binary tree                                                     8 roundings
  * pattern_dot_sum adds the nch chunks: a thread's chain of ceil(nch / 256) <= nch additions and the same tree (its 8 levels
    counted once more below)                                                                                   nch + 8 roundings
A term passes through at most  depth = 2 + cmax + run + 8 + nch + 8  roundings, each a factor (1 + t), |t| <= u, so
    |computed - exact| <= g(depth) sum_j sum_e |d_j| |a_e| |d_r(e)| <= depth * eps * |d|' |A| |d|
with the partition of csrc/gmrf_hip.hip (std_norm_chunks): nch = min(1024, max(1, ceil(n / 2048))), len = ceil(n / nch).
The exact value is evaluated here in longdouble (error ~ 2^-64 per operation, far below eps); without an 80-bit longdouble
`quadform_bound` adds the float64 evaluation's own (cmax + log2(nnz) + 2) u.  c = depth is a count of operations in the kernel's
source: nothing here was fitted to what the device returns.

The bound of the stage's sqmahal against a matrix assembled on the host
------------------------------------------------------------------------
gmrf_gn_posterior takes the quadratic form on ITS values of A = Q + noise J'J, the test on the oracle's (O.assemble_posterior of
the oracle's J at the same x): two float64 evaluations of one expression.  With Aabs = |Q| + noise |J|' |J|:
  * an entry q + noise sum_k J_ka J_kb with at most P products is formed in P + 2 roundings on either side:
        |A_dev - A_or| <= 2 g(P + 2) Aabs     from the arithmetic of the assembly,
  * the two J agree entry by entry within e_J = j_rel max |J| -- j_rel is the gate the tangent's own entry-by-entry test holds the
    device tangent to (1e-14 for the FEM tangents, 1e-13 for collocation), not a figure taken from this stage:
        |J_dev' J_dev - J_or' J_or| <= e_J (S' |J| + |J|' S) (1 + e_J / max|J|),    S = the pattern of J as ones.
So  |sqmahal_dev - sqmahal_or| <= depth eps |d|' Aabs |d| (1 + 2^-20)  +  2 (P + 2) eps |d|' Aabs |d|  +
                                 2 noise e_J (S |d|) . (|J| |d|) (1 + 2^-20)                                  (`stage_bound`).
"""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse as sp

EPS = 2.0 ** -52
LD = np.longdouble
LONGDOUBLE_OK = bool(np.finfo(np.longdouble).eps <= 2.0 ** -63)
SLACK = 1.0 + 2.0 ** -20


def chunks(n: int):
    """(nch, len) of the kernel's partition of the columns: a function of n only."""
    nch = min(1024, max(1, (n + 2047) // 2048))
    return nch, (n + nch - 1) // nch


def depth(A) -> int:
    """c of the bound: the roundings a term of the kernel's sum passes through (see the module docstring)."""
    A = sp.csc_matrix(A)
    n = A.shape[0]
    nch, length = chunks(n)
    cmax = int(np.max(np.diff(A.indptr)))
    run = (length + 255) // 256
    return 2 + cmax + run + 8 + nch + 8


def _terms(A, d, dtype):
    A = sp.csc_matrix(A)
    cols = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    return A.data.astype(dtype), d[A.indices], d[cols]


def sqmahal(A, x, z):
    """(z - x)' A (z - x) in longdouble, every stored entry of A (both triangles) once."""
    d = np.asarray(z, dtype=LD) - np.asarray(x, dtype=LD)
    a, dr, dc = _terms(A, d, LD)
    return LD(np.sum(a * dr * dc))


def abs_form(A, x, z):
    """|d|' |A| |d| in longdouble."""
    d = np.abs(np.asarray(z, dtype=LD) - np.asarray(x, dtype=LD))
    a, dr, dc = _terms(A, d, LD)
    return LD(np.sum(np.abs(a) * dr * dc))


def quadform_bound(A, x, z):
    """depth * eps * |d|' |A| |d| (plus the float64 evaluation's own error where longdouble is float64)."""
    A = sp.csc_matrix(A)
    c = depth(A)
    if not LONGDOUBLE_OK:
        c += (int(np.max(np.diff(A.indptr))) + int(math.ceil(math.log2(max(A.nnz, 2)))) + 2) / 2.0
    return float(c * EPS * abs_form(A, x, z))


def logdet_ld(A):
    """log det of a small dense positive definite matrix by an unblocked Cholesky in longdouble."""
    M = np.array(sp.csc_matrix(A).toarray(), dtype=LD)
    n = M.shape[0]
    s = LD(0)
    for j in range(n):
        piv = M[j, j]
        assert piv > 0
        l = M[j:, j] / np.sqrt(piv)
        s += np.log(piv)
        M[j:, j:] -= np.outer(l, l)
    return s


def nll(A, x, z, logdet=None):
    """0.5 (n log(2 pi) + sqmahal - logdet) in longdouble; logdet: given, or by `logdet_ld` (small n)."""
    n = sp.csc_matrix(A).shape[0]
    ld = logdet_ld(A) if logdet is None else LD(logdet)
    two_pi = LD(2) * LD("3.14159265358979323846264338327950288")
    return LD(0.5) * (LD(n) * np.log(two_pi) + sqmahal(A, x, z) - ld)


def stage_bound(Q, J, noise, x, z, j_rel):
    """The bound of the stage's sqmahal against the quadratic form on the host-assembled A = Q + noise J'J (module docstring)."""
    Q, J = sp.csc_matrix(Q), sp.csr_matrix(J)
    S = sp.csr_matrix((np.ones(J.nnz), J.indices, J.indptr), shape=J.shape)
    Ja = abs(J)
    Aabs = (abs(Q) + abs(noise) * (Ja.T @ Ja)).tocsc()
    Aabs.sort_indices()
    P = int((S.T @ S).max())
    d = np.abs(np.asarray(z, dtype=np.float64) - np.asarray(x, dtype=np.float64))
    form = float(abs_form(Aabs, np.zeros_like(d), d))
    e_j = j_rel * float(np.max(np.abs(J.data)))
    pattern = sp.csc_matrix((np.ones(Aabs.nnz), Aabs.indices, Aabs.indptr), shape=Aabs.shape)
    c = depth(pattern)
    return (c * EPS * form * SLACK + 2 * (P + 2) * EPS * form +
            2.0 * abs(noise) * e_j * float((S @ d) @ (Ja @ d)) * SLACK)
