"""NumPy restatement of the selected inverse on the pattern of Q (Takahashi recurrence on the block-tridiagonal factor).

With X_i = L_i^-1 and C_i = L_{i+1,i} (oracle.bt_oracle.tridiagonal_cholesky's chos / Cs), Sigma = Q^-1 on the block
tri-band follows from Sigma L = L^-T, block column i, from the last block upwards:
  Sigma_NN       = X_N^T X_N
  Sigma_{i+1,i}  = -Sigma_{i+1,i+1} C_i X_i
  Sigma_ii       = X_i^T (I + C_i^T Sigma_{i+1,i+1} C_i) X_i
(the form tests/test_gpu_parity.py's exact variances and oracle.bt_oracle.marginal_variances_exact use).
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np
import scipy.sparse as sp

from oracle import bt_oracle as O


def selected_blocks(F: O.TridiagonalCholeskyFactor, last_blocks: int = 0) -> Tuple[Dict[int, np.ndarray], Dict[int, np.ndarray]]:
    """(diag, low): diag[i] = Sigma_ii in full, low[i] = Sigma_{i+1,i}.  `last_blocks` > 0 stops the recurrence after that many
    diagonal blocks (as marginal_variances_exact does): diag then holds blocks N - last_blocks .. N - 1 only."""
    N, bs = F.n_blocks, F.block_size
    stop = 0 if last_blocks <= 0 else max(0, N - last_blocks)
    eye = np.eye(bs)
    X = O._chol_forward(F.chos[N - 1], eye)
    S = X.T @ X
    diag, low = {N - 1: 0.5 * (S + S.T)}, {}
    for i in range(N - 2, stop - 1, -1):
        C = F.Cs[i]
        X = O._chol_forward(F.chos[i], eye)
        Snext = diag[i + 1]
        low[i] = -(Snext @ C) @ X
        S = X.T @ ((eye + C.T @ (Snext @ C)) @ X)
        diag[i] = 0.5 * (S + S.T)
    return diag, low


def pattern_values(F: O.TridiagonalCholeskyFactor, S, last_blocks: int = 0):
    """Sigma at the stored entries of S (CSR order) and a mask of the entries the recurrence reached (with last_blocks > 0
    only the blocks it formed).  Also the scale sqrt(Sigma_rr Sigma_cc) of every entry (1 where not reached)."""
    S = sp.csr_matrix(S)
    S.sort_indices()
    diag, low = selected_blocks(F, last_blocks)
    bs = F.block_size
    rows = np.repeat(np.arange(S.shape[0]), np.diff(S.indptr))
    cols = S.indices.astype(np.int64)
    vals = np.full(S.nnz, np.nan)
    scale = np.ones(S.nnz)
    br, bc = rows // bs, cols // bs
    lr, lc = rows % bs, cols % bs
    for e in range(S.nnz):
        a, b = br[e], bc[e]
        if a == b and a in diag:
            vals[e] = diag[a][lr[e], lc[e]]
        elif a == b + 1 and b in low:
            vals[e] = low[b][lr[e], lc[e]]
        elif b == a + 1 and a in low:
            vals[e] = low[a][lc[e], lr[e]]
        else:
            continue
        if a in diag and b in diag:
            scale[e] = np.sqrt(diag[a][lr[e], lr[e]] * diag[b][lc[e], lc[e]])
    return vals, ~np.isnan(vals), scale


def entry_error(got, want, scale, mask=None) -> float:
    """max |got - want| / sqrt(Sigma_rr Sigma_cc) over the entries in `mask` (all by default)."""
    got, want, scale = np.asarray(got), np.asarray(want), np.asarray(scale)
    if mask is not None:
        got, want, scale = got[mask], want[mask], scale[mask]
    return float(np.max(np.abs(got - want) / scale))
