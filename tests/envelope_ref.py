"""The envelope bounds of the batched factorisation's 256-column panels, restated in NumPy from the SciPy pattern alone (shared by
tests/test_envelope_cpu.py and tests/test_gpu_envelope_bounds.py).

Per block i and 64-row tile t of the padded block: the rows that S_i = D_i - C C^T does not write (all rows of block 0, the rows
from rmax on otherwise; rmax = rows of the coupling blocks that hold entries, rounded up to 64) are still D_i's.
  lo[i][t]  smallest in-block column of the lower triangle of D_i in the tile's rows (the diagonal counts), rounded down to 64
  hi[i][t]  inside the 256-column panel of lo: the largest such column + 1, rounded up to 64; the panel's end where the tile lies in
            that panel itself
and 0 / bsp for every tile the product writes."""
import numpy as np
import scipy.sparse as sp


def padded_block(bs):
    t = -(-bs // 64)
    p = 1
    while p < t:
        p *= 2
    return 64 * p


def rmax_of(Q, N):
    n = Q.shape[0]
    bs = n // N
    coo = sp.coo_matrix(Q)
    sel = (coo.row // bs) == (coo.col // bs) + 1
    if not sel.any():
        return 64
    return min(padded_block(bs), -(-(int((coo.row[sel] % bs).max()) + 1) // 64) * 64)


def envelope(Q, N):
    """(lo, hi): int arrays [N][bsp / 64]."""
    n = Q.shape[0]
    bs = n // N
    bsp = padded_block(bs)
    nt = bsp // 64
    rmax = rmax_of(Q, N)
    coo = sp.coo_matrix(Q)
    lo = np.zeros((N, nt), np.int64)
    hi = np.full((N, nt), bsp, np.int64)
    for i in range(N):
        sel = (coo.row // bs == i) & (coo.col // bs == i) & (coo.row >= coo.col)
        r, c = coo.row[sel] - i * bs, coo.col[sel] - i * bs
        for t in range(nt):
            if i > 0 and 64 * t < rmax:
                continue
            ct = c[(r // 64) == t]
            first = min(int(ct.min()) if ct.size else 64 * t, 64 * t) // 64 * 64
            p0 = first // 256 * 256
            lo[i, t] = first
            if 64 * t < p0 + 256:
                hi[i, t] = min(p0 + 256, bsp)
            else:
                inside = ct[(ct >= p0) & (ct < p0 + 256)]
                hi[i, t] = -(-(int(inside.max()) + 1) // 64) * 64
    return lo, hi


def panel_bounds(lo, hi, i, p, tail_rides):
    """(kb, ke) of the row tiles below panel p of block i, relative to the panel; the last one trivial where it carries a tail."""
    nt = lo.shape[1]
    oa = 256 * p
    kb, ke = [], []
    for t in range(4 * p + 4, nt):
        b = min(max(int(lo[i, t]) - oa, 0), 256)
        e = min(max(int(hi[i, t]) - oa, b), 256) if oa <= lo[i, t] < oa + 256 else 256
        kb.append(b)
        ke.append(e)
    ub = list(kb)
    if tail_rides and kb:
        kb[-1], ke[-1] = 0, 256
    return kb, ke, ub


def units(lo, hi, i, p, tail_rides):
    """64-wide K units of panel p's product (K <= 64 (bn + 1): X_P is triangular) and of its rank-256 update (lower tiles)."""
    kb, ke, ub = panel_bounds(lo, hi, i, p, tail_rides)
    pp = sum(max(0, min(64 * (bn + 1), ke[bm]) - kb[bm]) // 64 for bm in range(len(kb)) for bn in range(4))
    upd = sum((256 - max(ub[bm], ub[bn])) // 64 for bm in range(len(ub)) for bn in range(bm + 1))
    return pp, upd


def no_structure_chain(bs=512, nb=3, seed=0):
    """Block tridiagonal, diagonally dominant, whose bounds are trivial for every panel: every row of a diagonal block meets the
    block's columns 0 and 255 (first and last column of the first panel), the coupling blocks hold entries in every row."""
    rng = np.random.default_rng(seed)
    n = bs * nb
    T = sp.lil_matrix((bs, bs))
    T.setdiag(-np.ones(bs - 1), -1)
    T[1:, 0] = -0.01
    T[256:, 255] = -0.01
    T = sp.csc_matrix(T)
    D = sp.kron(sp.eye(nb), T + T.T)
    Bc = sp.diags([-(0.5 + 0.5 * rng.random(bs)), -0.3 * np.ones(bs - 1)], [0, -1])
    Lo = sp.kron(sp.eye(nb, k=-1), Bc)
    Q = sp.csc_matrix(D + Lo + Lo.T + sp.diags(12.0 + rng.random(n)))
    Q.sort_indices()
    return Q
