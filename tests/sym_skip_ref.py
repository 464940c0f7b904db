"""A plain NumPy statement of the strict-lower mode of a square lower-only product (GemmArgs::strict_lower, csrc/gemm_f64.hpp):

  "nothing strictly above the ELEMENT diagonal of a square lower-only product is needed"

The bit says what a kernel MAY leave out.  The 64 x 64 LDS-DMA kernels (csrc/gemm_f64_dma.hpp) leave, in every diagonal tile,
  B stored [n][k] (the symmetric products of the factor): the six 16 x 16 MFMA blocks strictly above the tile's block diagonal,
  B stored [k][n]: the 32 x 32 quadrant rows 0 .. 31 x columns 32 .. 63 (there two MFMA blocks interleave their columns)
as C held them; every other kernel writes whole tiles.  Everything here follows that statement, not the kernels' code.

Masks are M x M booleans of one problem (T = 64: the tile of the grid).  Flops are counted per multiply-add of an output element
(2 per k): a computed element of a tile costs the tile's K range.
"""
from __future__ import annotations

import numpy as np

T = 64
Q = 32          # a wave's quadrant
BLK = 16        # an MFMA block


def _rc(M):
    return np.arange(M)[:, None], np.arange(M)[None, :]


def must_write(M):
    """Elements a strict-lower launch must write: row >= col (all of them lie in computed tiles, bn <= bm)."""
    r, c = _rc(M)
    return r >= c


def may_write(M):
    """Elements it may write: the whole tiles with bn <= bm."""
    r, c = _rc(M)
    return (c // T) <= (r // T)


def skipped(M, b_n=0):
    """What the 64 x 64 LDS-DMA family leaves out of every diagonal tile."""
    r, c = _rc(M)
    diag = (r // T) == (c // T)
    if b_n:
        return diag & ((r % T) < Q) & ((c % T) >= Q)
    return diag & (((r % T) // BLK) < ((c % T) // BLK))


def unchanged(M, dma64, b_n=0):
    """Elements a strict-lower launch must leave bit-unchanged: the tiles with bn > bm, and (64 x 64 LDS-DMA family) what it skips."""
    u = ~may_write(M)
    return (u | skipped(M, b_n)) if dma64 else u


def diag_share(b_n=0):
    """Share of a diagonal tile's MFMAs the strict-lower mode of the 64 x 64 LDS-DMA family executes."""
    return 0.75 if b_n else 10.0 / 16.0


def tile_k(K, kb, bm, bn):
    """K range length of tile (bm, bn) of a triangular grid: from max(kb[bm], kb[bn]) (staircase bounds, or None) to K."""
    lo = 0 if kb is None else max(kb[bm], kb[bn])
    return max(K - lo, 0)


def executed_flops(M, K, kb=None, strict=False, b_n=0):
    """Multiply-add flops a triangular grid of 64 x 64 tiles executes: every tile bn <= bm whole, a diagonal tile diag_share of it
    in the strict-lower mode of the 64 x 64 LDS-DMA family."""
    nt = M // T
    f = 0.0
    for bm in range(nt):
        for bn in range(bm + 1):
            share = diag_share(b_n) if (strict and bm == bn) else 1.0
            f += 2.0 * T * T * tile_k(K, kb, bm, bn) * share
    return f


def executed_flops_brute(M, K, kb=None, strict=False, b_n=0):
    """The same, element by element: an element is computed if its tile is on or below the block diagonal and (strict) it is not
    skipped; it then costs its tile's K range."""
    comp = may_write(M) & ~(skipped(M, b_n) if strict else np.zeros((M, M), bool))
    f = 0.0
    for r in range(M):
        for c in range(M):
            if comp[r, c]:
                f += 2.0 * tile_k(K, kb, r // T, c // T)
    return f


def k_units(M, K, kb=None):
    """(all, diagonal) 64-wide tile-K units of a triangular grid."""
    nt = M // T
    every = sum(tile_k(K, kb, bm, bn) for bm in range(nt) for bn in range(bm + 1)) / T
    diag = sum(tile_k(K, kb, b, b) for b in range(nt)) / T
    return every, diag
