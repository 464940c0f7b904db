"""A plain NumPy statement of the GEMM descriptor (GemmArgs, csrc/gemm_f64.hpp) for the descriptor-level kernel tests.

  C_z[m][n] = beta * D_zp[m][n] + alpha * sum_k a_z(m, k) b_z(k, n),      z < batch, zi = z % nb1, zp = z // nb1
  A_z at A + zi strideA + zp pA (B, C alike), D_zp at D + zp pD (the inner items of a problem share their addend)

and the tail row / direct output of the LDS-DMA kernel's TAIL / DOUT variants.  The module also builds the test
buffers: whatever the descriptor says is not part of the operation holds a sentinel (NaN in inputs, a NaN with a
payload of its own in outputs), and K ranges that the tri flags / K bounds exclude are NaN too, at the granularity of
the tile of the kernel under test (a kernel reads whole tiles: inside a tile that is read, declared zeros are real
zeros).  Everything here follows the comments of the headers (the contract), not the kernels' code.

Tolerance, for every written element (u = 2^-53):

  |got - ref| <= (K + 4) u (|alpha| (|a| @ |b|) + |beta| |D|)

gamma_K-style bound of a K-term dot product in ANY summation order, with or without FMA (Higham, Accuracy and Stability
of Numerical Algorithms, section 3.1: K u to first order; the mantissa of the second-order term is covered by the + 4),
one rounding each for alpha * sum, beta * D and their sum, and the reference's own error (longdouble, eps 2^-63: K 2^-63
relative to the magnitude sum, far below one u).  Without an 80-bit longdouble the reference is no better than the
kernel and the factor is (2 K + 4).  The magnitude sum itself is formed in float64 (relative error K u of a factor that
multiplies u: second order) and enlarged by 1 + 2^-40 to stay on the safe side of that.
"""
from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

U = 2.0 ** -53
LONGDOUBLE_OK = bool(np.finfo(np.longdouble).eps <= 2.0 ** -63)
OUT_SENTINEL = np.uint64(0x7FF8DEAD0000BEEF)          # a NaN: outputs are compared as bits

TRI_A_LOWER, TRI_A_UPPER, TRI_B_LOWER, TRI_B_UPPER = 1, 2, 4, 8

# routes of gmrf_test_gemm_desc and the families it reports
REG, BIG, LL, DMA64, DMA128x64, DMA64x128, TAIL, AUTO = range(8)
FAM_REG16, FAM_REG32, FAM_BIG, FAM_LL, FAM_DMA64, FAM_DMA128x64, FAM_DMA64x128, FAM_TAIL, FAM_DOUT = range(1, 10)
FAM_SINGLE = 256
FAM_TILE = {FAM_REG16: (64, 64), FAM_REG32: (64, 64), FAM_BIG: (128, 128), FAM_LL: (32, 32), FAM_DMA64: (64, 64),
            FAM_DMA128x64: (128, 64), FAM_DMA64x128: (64, 128), FAM_TAIL: (64, 64), FAM_DOUT: (64, 64)}
# tiles whose OUTPUT a lower-only launch writes: the LDS-DMA kernels idle the 64 x 64 parts above the diagonal of a wide tile
FAM_OUT_TILE = {**FAM_TILE, FAM_DMA128x64: (64, 64), FAM_DMA64x128: (64, 64)}


def tol_factor(K):
    return (K + 4) if LONGDOUBLE_OK else (2 * K + 4)


@dataclass(frozen=True)
class Desc:
    M: int
    N: int
    K: int
    transA: int = 0          # A stored [k][m]
    b_n: int = 0             # B stored [k][n] (else [n][k])
    tri: int = 0
    lower_only: int = 0
    batch: int = 1
    nb1: int = 1
    lda: int = 0
    ldb: int = 0
    ldc: int = 0
    ldd: int = 0
    sA: int = 0
    sB: int = 0
    sC: int = 0
    pA: int = 0
    pB: int = 0
    pC: int = 0
    pD: int = 0
    ptA: int = 0
    ptC: int = 0
    ptD: int = 0
    o_j0: int = 0
    o_n: int = 0
    o_cols: int = 0
    o_ld: int = 0
    o_k: int = 0
    alpha: float = 1.0
    beta: float = 0.0
    tbeta: float = 0.0
    has_D: bool = False
    tail: int = 0            # 0 none, 1 row M of A / C / D, 2 operands of its own (tA / tC / tD)
    has_tD: bool = False
    dout: bool = False
    kb_m: tuple = None
    kb_n: tuple = None
    ke_n: tuple = None

    @property
    def np_(self):
        return self.batch // self.nb1

    @property
    def rows(self):          # rows of A (stored [m][k]), C and D
        return self.M + (1 if self.tail == 1 else 0)

    def desc_array(self):
        return np.array([self.M, self.N, self.K, self.transA, self.b_n, self.tri, self.lower_only, self.batch, self.nb1,
                         self.lda, self.ldb, self.ldc, self.ldd, self.sA, self.sB, self.sC, self.pA, self.pB, self.pC, self.pD,
                         self.ptA, self.ptC, self.ptD, self.o_j0, self.o_n, self.o_cols, self.o_ld, self.o_k], dtype=np.int64)


def _pad_ld(w):
    """Even, not a multiple of 64, wider than w."""
    ld = w + 6
    if ld % 64 == 0:
        ld += 2
    return ld


def make(M, N, K, layout="inter", **kw):
    """A descriptor with its strides laid out.  layout 'inter': the rows of all problems interleave in one buffer (problem z's
    row r at r ld + z (w + 2), as the handles' panels lie), 'stack': one problem after the other with a gap, 'tight': no padding."""
    d = Desc(M, N, K, **kw)
    wa = M if d.transA else K
    wb = N if d.b_n else K
    rows_a = K if d.transA else d.rows
    rows_b = K if d.b_n else N
    f = {}
    if layout == "inter":
        for nm, w in (("A", wa), ("B", wb), ("C", N)):
            W = w + 2
            f["ld" + nm.lower()] = _pad_ld(d.batch * W)
            f["s" + nm] = W
            f["p" + nm] = d.nb1 * W
        f["ldd"] = _pad_ld(d.np_ * (N + 4)) + 4
        f["pD"] = N + 4
    else:
        gap = 0 if layout == "tight" else 10
        for nm, w, r in (("A", wa, rows_a), ("B", wb, rows_b), ("C", N, d.rows)):
            ld = kw.get("ld" + nm.lower(), w if layout == "tight" else _pad_ld(w))
            f["ld" + nm.lower()] = ld
            f["s" + nm] = r * ld + gap
            f["p" + nm] = d.nb1 * (r * ld + gap)
        f["ldd"] = N if layout == "tight" else _pad_ld(N) + 8
        f["pD"] = d.rows * f["ldd"] + (0 if layout == "tight" else 22)
    if not d.has_D:
        f["ldd"] = 0
        f["pD"] = 0
    if d.tail == 2:
        f.update(ptA=K + 6, ptC=N + 4, ptD=N + 8)
    if d.dout:
        f.setdefault("o_n", 0)
    f = {k: v for k, v in f.items() if k not in kw}
    return replace(d, **f)


# ------------------------------------------------------------------------------------------------ sizes
def need(d):
    """Elements each buffer must hold: the furthest element the descriptor addresses, plus one."""
    zi, zo = d.nb1 - 1, d.np_ - 1
    n = {
        "A": zi * d.sA + zo * d.pA + ((d.K - 1) * d.lda + d.M if d.transA else (d.rows - 1) * d.lda + d.K),
        "B": zi * d.sB + zo * d.pB + ((d.K - 1) * d.ldb + d.N if d.b_n else (d.N - 1) * d.ldb + d.K),
        "C": zi * d.sC + zo * d.pC + (d.rows - 1) * d.ldc + d.N,
    }
    if d.has_D:
        n["D"] = zo * d.pD + (d.rows - 1) * d.ldd + d.N
    if d.tail == 2:
        n["tA"] = zo * d.ptA + d.K
        n["tC"] = zo * d.ptC + d.N
        if d.has_tD:
            n["tD"] = zo * d.ptD + d.N
    if d.dout:
        n["samples"] = (zo * d.o_k + d.o_k - 1) * d.o_ld + d.o_j0 + d.o_cols if d.o_k > 0 and d.o_cols > 0 else 0
        n["mean"] = zo * d.o_n + d.o_j0 + d.o_cols if d.o_cols > 0 else 0
    return n


def _grid(rows, cols, ld):
    return np.arange(rows, dtype=np.int64)[:, None] * ld + np.arange(cols, dtype=np.int64)[None, :]


def index_maps(d):
    """Per buffer and problem: the flat indices of the logical elements (the generator's own statement of the layout)."""
    out = {k: [] for k in ("A", "B", "C", "D", "tA", "tC", "tD")}
    for z in range(d.batch):
        zi, zp = z % d.nb1, z // d.nb1
        a = _grid(d.K, d.M, d.lda).T if d.transA else _grid(d.rows, d.K, d.lda)            # [row of op(A) (+ tail)][k]
        b = _grid(d.K, d.N, d.ldb) if d.b_n else _grid(d.N, d.K, d.ldb).T                  # [k][n]
        out["A"].append(zi * d.sA + zp * d.pA + a)
        out["B"].append(zi * d.sB + zp * d.pB + b)
        out["C"].append(zi * d.sC + zp * d.pC + _grid(d.rows, d.N, d.ldc))
    for zp in range(d.np_):
        if d.has_D:
            out["D"].append(zp * d.pD + _grid(d.rows, d.N, d.ldd))
        if d.tail == 2:
            out["tA"].append(zp * d.ptA + np.arange(d.K, dtype=np.int64))
            out["tC"].append(zp * d.ptC + np.arange(d.N, dtype=np.int64))
            if d.has_tD:
                out["tD"].append(zp * d.ptD + np.arange(d.N, dtype=np.int64))
    return out


# ------------------------------------------------------------------------------------------------ K ranges
def tile_range(d, BM, BN, bm, bn):
    """K range of tile (bm, bn) of BM x BN (the spec of the headers: bounds per 64-wide part, a wider tile starts at its
    first part's bound and ends at its last part's; a 32-wide tile takes its 64-wide part's)."""
    kb, ke = 0, d.K
    if d.tri & TRI_A_LOWER: ke = min(ke, (bm + 1) * BM)
    if d.tri & TRI_A_UPPER: kb = max(kb, bm * BM)
    if d.tri & TRI_B_LOWER: kb = max(kb, bn * BN)
    if d.tri & TRI_B_UPPER: ke = min(ke, (bn + 1) * BN)
    if d.kb_m is not None: kb = max(kb, d.kb_m[(bm * BM) // 64])
    if d.kb_n is not None: kb = max(kb, d.kb_n[(bn * BN) // 64])
    if d.ke_n is not None: ke = min(ke, d.ke_n[((bn + 1) * BN - 1) // 64])
    return kb, max(ke, kb)


def tile_computed(d, BM, BN, bm, bn):
    """lower_only: a tile is worked on when it touches the block lower triangle."""
    return (not d.lower_only) or bn * BN <= bm * BM + BM - 1


def tail_owner(d, bn):
    """Row tile (64 x 64) that carries the tail of column tile bn: the diagonal tile of a triangular grid, else the last."""
    return bn if (d.lower_only and d.M == d.N) else d.M // 64 - 1


def read_masks(d, tile):
    """(M x K, K x N, K) booleans: elements of op(A), op(B) and the tail row some tile of the launch reads."""
    BM, BN = tile
    ra = np.zeros((d.M, d.K), bool)
    rb = np.zeros((d.K, d.N), bool)
    rt = np.zeros(d.K, bool)
    for bm in range(d.M // BM):
        for bn in range(d.N // BN):
            if not tile_computed(d, BM, BN, bm, bn):
                continue
            kb, ke = tile_range(d, BM, BN, bm, bn)
            ra[bm * BM:(bm + 1) * BM, kb:ke] = True
            rb[kb:ke, bn * BN:(bn + 1) * BN] = True
    if d.tail:
        for bn in range(d.N // 64):
            bms = range(d.M // 64) if d.dout else [tail_owner(d, bn)]
            for bm in bms:
                kb, ke = tile_range(d, 64, 64, bm, bn)
                rt[kb:ke] = True
    return ra, rb, rt


def elem_bounds(d):
    """Brute force, per element (m, n): the k range [lo, hi) outside which the term a(m,k) b(k,n) is declared zero."""
    m = np.arange(d.M)[:, None] + np.zeros((1, d.N), int)
    n = np.arange(d.N)[None, :] + np.zeros((d.M, 1), int)
    lo = np.zeros((d.M, d.N), int)
    hi = np.full((d.M, d.N), d.K)
    if d.tri & TRI_A_LOWER: hi = np.minimum(hi, m + 1)
    if d.tri & TRI_A_UPPER: lo = np.maximum(lo, m)
    if d.tri & TRI_B_LOWER: lo = np.maximum(lo, n)
    if d.tri & TRI_B_UPPER: hi = np.minimum(hi, n + 1)
    if d.kb_m is not None: lo = np.maximum(lo, np.asarray(d.kb_m)[m // 64])
    if d.kb_n is not None: lo = np.maximum(lo, np.asarray(d.kb_n)[n // 64])
    if d.ke_n is not None: hi = np.minimum(hi, np.asarray(d.ke_n)[n // 64])
    return lo, hi


def written_mask(d, fam):
    """M x N boolean: elements of C the kernel family writes (lower_only: the tiles of ITS size with bn <= bm)."""
    T, _ = FAM_OUT_TILE[fam & 255]
    w = np.ones((d.M, d.N), bool)
    if d.lower_only:
        w = (np.arange(d.N)[None, :] // T) <= (np.arange(d.M)[:, None] // T)
    return w


def may_write_mask(d, fam):
    """What a lower-only launch MAY write: the 64 x 64 tiles with bn <= bm (the 128 x 128 kernel: its own tiles)."""
    T = max(64, FAM_OUT_TILE[fam & 255][0])
    w = np.ones((d.M, d.N), bool)
    if d.lower_only:
        w = (np.arange(d.N)[None, :] // T) <= (np.arange(d.M)[:, None] // T)
    return w


def empty_mask(d, fam):
    """M x N boolean: elements in tiles (of the kernel's size) whose K range is empty."""
    BM, BN = FAM_TILE[fam & 255]
    e = np.zeros((d.M, d.N), bool)
    for bm in range(d.M // BM):
        for bn in range(d.N // BN):
            kb, ke = tile_range(d, BM, BN, bm, bn)
            if ke <= kb:
                e[bm * BM:(bm + 1) * BM, bn * BN:(bn + 1) * BN] = True
    return e


# ------------------------------------------------------------------------------------------------ data
def zero_masks(d):
    """Declared zeros of op(A) (M x K) and op(B) (K x N), per element."""
    m = np.arange(d.M)[:, None]
    k = np.arange(d.K)[None, :]
    za = np.zeros((d.M, d.K), bool)
    if d.tri & TRI_A_LOWER: za |= k > m
    if d.tri & TRI_A_UPPER: za |= k < m
    if d.kb_m is not None: za |= k < np.asarray(d.kb_m)[m // 64]
    k = np.arange(d.K)[:, None]
    n = np.arange(d.N)[None, :]
    zb = np.zeros((d.K, d.N), bool)
    if d.tri & TRI_B_LOWER: zb |= k < n
    if d.tri & TRI_B_UPPER: zb |= k > n
    if d.kb_n is not None: zb |= k < np.asarray(d.kb_n)[n // 64]
    if d.ke_n is not None: zb |= k >= np.asarray(d.ke_n)[n // 64]
    return za, zb


_DATA = {}


def logical(d, seed):
    """Random logical operands of every problem (memoised; the same for every descriptor of one seed and shape, whatever
    its layout and flags): op(A) with its tail row, op(B), C as it comes in, D, the tail's own operands."""
    key = (seed, d.M, d.N, d.K, d.batch, d.nb1)
    if key not in _DATA:
        rng = np.random.default_rng(seed)
        dat = {k: [] for k in ("A", "B", "C", "D", "tA", "tC", "tD")}
        for _ in range(d.batch):
            dat["A"].append(rng.standard_normal((d.M + 1, d.K)))
            dat["B"].append(rng.standard_normal((d.K, d.N)))
            dat["C"].append(rng.standard_normal((d.M + 1, d.N)))
        for _ in range(d.np_):
            dat["D"].append(rng.standard_normal((d.M + 1, d.N)))
            dat["tA"].append(rng.standard_normal(d.K))
            dat["tC"].append(rng.standard_normal(d.N))
            dat["tD"].append(rng.standard_normal(d.N))
        for v in dat.values():
            for a in v:
                a.setflags(write=False)
        _DATA[key] = dat
    return _DATA[key]


def pick(d, data, z):
    """Problem z of a batch as a launch of its own: (descriptor, data)."""
    zp = z // d.nb1
    d1 = replace(d, batch=1, nb1=1)
    dat = {k: [data[k][z]] for k in ("A", "B", "C")}
    dat.update({k: [data[k][zp]] for k in ("D", "tA", "tC", "tD")})
    return d1, dat


def build(d, data, tile):
    """The buffers of a launch.  Inputs: NaN everywhere, then the logical operands (declared zeros as real zeros), then NaN
    again on what no tile of size `tile` reads.  Outputs: the sentinel, then (only where the operation reads C: beta != 0 without
    a D) the incoming values; NaN otherwise."""
    sz = need(d)
    ix = index_maps(d)
    za, zb = zero_masks(d)
    ra, rb, rt = read_masks(d, tile)
    buf = {}
    A = np.full(sz["A"], np.nan)
    B = np.full(sz["B"], np.nan)
    C = np.full(sz["C"], np.nan)
    C.view(np.uint64)[:] = OUT_SENTINEL
    for z in range(d.batch):
        a = np.where(za, 0.0, data["A"][z][:d.M])
        a = np.where(ra, a, np.nan)
        if d.tail == 1:
            a = np.vstack([a, np.where(rt, data["A"][z][d.M], np.nan)[None, :]])
        A[ix["A"][z]] = a
        b = np.where(zb, 0.0, data["B"][z])
        B[ix["B"][z]] = np.where(rb, b, np.nan)
        c_read = d.beta != 0.0 and not d.has_D
        C[ix["C"][z]] = data["C"][z][:d.rows] if c_read else np.nan
    buf.update(A=A, B=B, C=C)
    if d.has_D:
        D = np.full(sz["D"], np.nan)
        for zp in range(d.np_):
            D[ix["D"][zp]] = data["D"][zp][:d.rows]
        buf["D"] = D
    if d.tail == 2:
        tA = np.full(sz["tA"], np.nan)
        tC = np.full(sz["tC"], np.nan)
        tC.view(np.uint64)[:] = OUT_SENTINEL
        for zp in range(d.np_):
            tA[ix["tA"][zp]] = np.where(rt, data["tA"][zp], np.nan)
            tC[ix["tC"][zp]] = data["tC"][zp] if (d.tbeta != 0.0 and not d.has_tD) else np.nan
        buf.update(tA=tA, tC=tC)
        if d.has_tD:
            tD = np.full(sz["tD"], np.nan)
            for zp in range(d.np_):
                tD[ix["tD"][zp]] = data["tD"][zp]
            buf["tD"] = tD
    if d.dout:
        for nm in ("samples", "mean"):
            o = np.full(sz[nm] + 7, np.nan)               # (a few elements past the furthest: they stay untouched too)
            o.view(np.uint64)[:] = OUT_SENTINEL
            buf[nm] = o
    for nm in ("kb_m", "kb_n", "ke_n"):
        v = getattr(d, nm)
        if v is not None:
            buf[nm] = np.asarray(v, dtype=np.int32)
    return buf


# ------------------------------------------------------------------------------------------------ reference
_REF = {}


def _key(d):
    # what the values depend on (not the layout)
    return (d.M, d.N, d.K, d.tri, d.batch, d.nb1, d.alpha, d.beta, d.tbeta, d.has_D, d.tail, d.has_tD, d.dout,
            d.lower_only and d.M == d.N, d.kb_m, d.kb_n, d.ke_n)


def reference(d, data, seed=None):
    """Per problem: ref (rows x N, longdouble), mag (rows x N, float64: the magnitude sum of the tolerance) and for the tail of its
    own tref / tmag (N).  Row M of ref / mag is the tail row when the tail is row M.  Memoised per (seed, descriptor values)."""
    key = (seed, _key(d)) if seed is not None else None
    if key is not None and key in _REF:
        return _REF[key]
    L = np.longdouble
    za, zb = zero_masks(d)
    out = []
    for z in range(d.batch):
        zp = z // d.nb1
        a = np.where(za, 0.0, data["A"][z][:d.M])
        b = np.where(zb, 0.0, data["B"][z])
        addend = data["D"][zp] if d.has_D else data["C"][z]
        ref = L(d.alpha) * (a.astype(L) @ b.astype(L))
        mag = abs(d.alpha) * (np.abs(a) @ np.abs(b))
        if d.beta != 0.0:
            ref = ref + L(d.beta) * addend[:d.M].astype(L)
            mag = mag + abs(d.beta) * np.abs(addend[:d.M])
        r = {"ref": ref, "mag": mag * (1.0 + 2.0 ** -40)}
        if d.tail:
            ta = data["A"][z][d.M] if d.tail == 1 else data["tA"][zp]
            tb = d.beta if d.tail == 1 else d.tbeta
            td = addend[d.M] if d.tail == 1 else (data["tD"][zp] if d.has_tD else data["tC"][zp])
            tref = np.zeros(d.N, L)
            tmag = np.zeros(d.N)
            for bn in range(d.N // 64):
                kb, ke = tile_range(d, 64, 64, tail_owner(d, bn), bn)
                s = slice(bn * 64, bn * 64 + 64)
                tref[s] = L(d.alpha) * (ta[kb:ke].astype(L) @ b[kb:ke, s].astype(L))
                tmag[s] = abs(d.alpha) * (np.abs(ta[kb:ke]) @ np.abs(b[kb:ke, s]))
            if tb != 0.0:
                tref = tref + L(tb) * td.astype(L)
                tmag = tmag + abs(tb) * np.abs(td)
            r["tref"] = tref
            r["tmag"] = tmag * (1.0 + 2.0 ** -40)
        out.append(r)
    if key is not None:
        _REF[key] = out
    return out


def within(got, ref, mag, K, extra=0):
    """got within the derived bound of ref, element by element (a NaN is not)."""
    err = np.abs(got.astype(np.longdouble) - ref)
    return bool(np.all(err <= (tol_factor(K) + extra) * U * mag))


def worst(got, ref, mag, K):
    """Largest error in units of the bound (to print before asserting)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.abs(got.astype(np.longdouble) - ref) / (tol_factor(K) * U * np.maximum(mag, np.finfo(float).tiny))
    return float(np.nanmax(q)) if not np.isnan(q).all() else float("nan")


def staircase(M, N, K):
    """Monotone bounds in multiples of 64 like the coupling blocks': kb_m grows with the row tile, kb_n and ke_n with the column
    tile; with K = 256 the last row tile's start (192) meets column tile 0's end (64): empty ranges, and the steps of 64 split
    every 128-wide tile."""
    kb_m = tuple(min(64 * t, K - 64) for t in range(M // 64))
    kb_n = tuple(min(64 * (t // 2), K - 64) for t in range(N // 64))
    ke_n = tuple(min(64 * (t + 1), K) for t in range(N // 64))
    return kb_m, kb_n, ke_n
