"""NumPy restatement of the two-ended ("twisted") block-tridiagonal factorisation Q = T T^T.

Blocks are 0-based; D_i = Q[i, i], B_i = Q[i, i-1]; m is the meeting block.
  top chain (i < m):     L_i L_i^T = D_i - G_i G_i^T,            G_i = B_i L_{i-1}^-T
  bottom chain (i > m):  U_i U_i^T = D_i - H_i H_i^T,            H_i = B_{i+1}^T U_{i+1}^-T   (U_i upper triangular)
  meeting block:         L_m L_m^T = D_m - G_m G_m^T - H_m H_m^T
T has the diagonal blocks L_i (i <= m) / U_i (i > m), T[i, i-1] = G_i (1 <= i <= m) and T[i, i+1] = H_i (m <= i < N-1).

The two chains come from the reference-order oracle (oracle.bt_oracle.tridiagonal_cholesky): the top one factors Q's
leading blocks 0 .. m-1, the bottom one the fully index-reversed trailing matrix over blocks N-1 .. m+1, so that
U_i = J L'_j J (J: the flip inside a block, j = N-1-i) and H_i = J C'_{j-1} J for i > m.  The meeting block, the sweeps
and the seeded selected inversion are done here.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

from oracle import bt_oracle as O


@dataclass
class TwistedFactor:
    N: int                       # total size n (the reference's convention)
    m: int                       # meeting block
    diag: List[np.ndarray]       # T_ii: L_i (i <= m, lower) or U_i (i > m, upper)
    G: Dict[int, np.ndarray]     # G_i = T[i, i-1], 1 <= i <= m
    H: Dict[int, np.ndarray]     # H_i = T[i, i+1], m <= i < N-1

    @property
    def n_blocks(self) -> int:
        return len(self.diag)

    @property
    def block_size(self) -> int:
        return self.diag[0].shape[0]

    def block(self, kind: str, i: int) -> np.ndarray:
        """What gmrf_bt_get_block returns: kind "L" -> T_ii, "C" -> G_{i+1} (i < m) or H_i (i >= m), "LINV" -> T_ii^-1."""
        if kind == "L":
            return self.diag[i]
        if kind == "C":
            return self.G[i + 1] if i < self.m else self.H[i]
        return np.linalg.inv(self.diag[i])


def _flip(A: np.ndarray) -> np.ndarray:
    return A[::-1, ::-1]


def auto_meet(n_blocks: int) -> int:
    """The fall-back of the automatic choice for short chains (N < 3: the reference order)."""
    return n_blocks - 1


def tridiagonal_cholesky(A, n_blocks: int, m: int) -> TwistedFactor:
    A = sp.csr_matrix(A)
    n = A.shape[0]
    bs = n // n_blocks
    N = n_blocks
    if not 0 <= m <= N - 1:
        raise ValueError("meeting block out of range")

    def dense(bi, bj):
        return A[bi * bs:(bi + 1) * bs, bj * bs:(bj + 1) * bs].toarray()

    diag: List[np.ndarray] = [None] * N
    G: Dict[int, np.ndarray] = {}
    H: Dict[int, np.ndarray] = {}
    if m > 0:
        Ft = O.tridiagonal_cholesky(A[:m * bs, :m * bs], m)
        for i in range(m):
            diag[i] = Ft.chos[i]
        for i in range(1, m):
            G[i] = Ft.Cs[i - 1]
        G[m] = sla.solve_triangular(Ft.chos[m - 1], dense(m, m - 1).T, lower=True).T          # B_m L_{m-1}^-T
    S = np.tril(dense(m, m))
    S = S + np.tril(S, -1).T
    if m > 0:
        S = S - G[m] @ G[m].T
    if m < N - 1:
        Nb = N - 1 - m
        R = A[(m + 1) * bs:, (m + 1) * bs:][::-1, ::-1]
        Fb = O.tridiagonal_cholesky(sp.csr_matrix(R), Nb)
        for j in range(Nb):
            diag[N - 1 - j] = _flip(Fb.chos[j])
        for j in range(1, Nb):
            H[N - 1 - j] = _flip(Fb.Cs[j - 1])                                                  # T[N-1-j, N-j]
        U = diag[m + 1]
        Bt = dense(m + 1, m).T                                                                  # Q[m, m+1]
        H[m] = sla.solve_triangular(U, Bt.T, lower=False).T                                     # B_{m+1}^T U_{m+1}^-T
        S = S - H[m] @ H[m].T
    try:
        diag[m] = sla.cholesky(S, lower=True)
    except sla.LinAlgError:
        raise O.NotPositiveDefinite(m + 1) from None
    return TwistedFactor(n, m, diag, G, H)


def dense_T(F: TwistedFactor) -> np.ndarray:
    N, bs = F.n_blocks, F.block_size
    T = np.zeros((F.N, F.N))
    for i in range(N):
        T[i * bs:(i + 1) * bs, i * bs:(i + 1) * bs] = F.diag[i]
    for i, Gi in F.G.items():
        T[i * bs:(i + 1) * bs, (i - 1) * bs:i * bs] = Gi
    for i, Hi in F.H.items():
        T[i * bs:(i + 1) * bs, (i + 1) * bs:(i + 2) * bs] = Hi
    return T


def _chunks(b: np.ndarray, N: int, bs: int):
    return [b[i * bs:(i + 1) * bs] for i in range(N)]


def forward_solve(F: TwistedFactor, b: np.ndarray) -> np.ndarray:
    """y = T^-1 b: the top runs down, the bottom runs up, then the meeting block."""
    N, bs, m = F.n_blocks, F.block_size, F.m
    bc = _chunks(np.asarray(b, dtype=np.float64), N, bs)
    y = [None] * N
    for i in range(m):
        r = bc[i] - (F.G[i] @ y[i - 1] if i > 0 else 0.0)
        y[i] = sla.solve_triangular(F.diag[i], r, lower=True)
    for i in range(N - 1, m, -1):
        r = bc[i] - (F.H[i] @ y[i + 1] if i < N - 1 else 0.0)
        y[i] = sla.solve_triangular(F.diag[i], r, lower=False)
    r = bc[m].copy()
    if m > 0:
        r = r - F.G[m] @ y[m - 1]
    if m < N - 1:
        r = r - F.H[m] @ y[m + 1]
    y[m] = sla.solve_triangular(F.diag[m], r, lower=True)
    return np.concatenate(y, axis=0)


def backward_solve(F: TwistedFactor, y: np.ndarray) -> np.ndarray:
    """x = T^-T y: the meeting block first, then both halves outward."""
    N, bs, m = F.n_blocks, F.block_size, F.m
    yc = _chunks(np.asarray(y, dtype=np.float64), N, bs)
    x = [None] * N
    x[m] = sla.solve_triangular(F.diag[m], yc[m], lower=True, trans="T")
    for i in range(m - 1, -1, -1):
        x[i] = sla.solve_triangular(F.diag[i], yc[i] - F.G[i + 1].T @ x[i + 1], lower=True, trans="T")
    for i in range(m + 1, N):
        x[i] = sla.solve_triangular(F.diag[i], yc[i] - F.H[i - 1].T @ x[i - 1], lower=False, trans="T")
    return np.concatenate(x, axis=0)


def ldiv(F: TwistedFactor, b: np.ndarray) -> np.ndarray:
    return backward_solve(F, forward_solve(F, b))


def sample(F: TwistedFactor, mean: np.ndarray, Z: np.ndarray) -> np.ndarray:
    X = backward_solve(F, Z)
    return X + (mean[:, None] if Z.ndim == 2 else mean)


def logdet(F: TwistedFactor) -> float:
    return 2.0 * float(sum(np.log(np.abs(np.diag(D))).sum() for D in F.diag))


def marginal_variances_exact(F: TwistedFactor) -> np.ndarray:
    """Selected inversion from the meeting block outward:
    Sigma_mm = L_m^-T L_m^-1;  Sigma_ii = L_i^-T (I + G_{i+1}^T Sigma_{i+1} G_{i+1}) L_i^-1  (i < m);
    Sigma_ii = U_i^-T (I + H_{i-1}^T Sigma_{i-1} H_{i-1}) U_i^-1  (i > m)."""
    N, bs, m = F.n_blocks, F.block_size, F.m
    out = np.empty(F.N)
    eye = np.eye(bs)

    def inv(i):
        return sla.solve_triangular(F.diag[i], eye, lower=i <= m)

    Xm = inv(m)
    Sm = Xm.T @ Xm
    out[m * bs:(m + 1) * bs] = np.diag(Sm)
    S = Sm
    for i in range(m - 1, -1, -1):
        X = inv(i)
        Gc = F.G[i + 1]
        S = X.T @ (eye + Gc.T @ S @ Gc) @ X
        S = 0.5 * (S + S.T)
        out[i * bs:(i + 1) * bs] = np.diag(S)
    S = Sm
    for i in range(m + 1, N):
        X = inv(i)
        Hc = F.H[i - 1]
        S = X.T @ (eye + Hc.T @ S @ Hc) @ X
        S = 0.5 * (S + S.T)
        out[i * bs:(i + 1) * bs] = np.diag(S)
    return out
