"""The sparse products Y = S X restated for the tests (no GPU, no library):

* the tile plan of the node-major kernels and the two route functions, written from the comments and constants of
  csr_spmm_tiles / csr_spmm_tiles_pad / csr_spmv_tiles and their launchers (NOT from the host code's control flow: the
  CPU test compares the two);
* the reference product in np.longdouble from the values the kernel sees, with the row-wise bound
      |y_i - yhat_i| <= (L_i + 2) 2^-53 sum_e |a_e| |x_e|
  of a length-L_i chain or tree of fp64 fused multiply-adds (every term passes one rounding of its product-and-add and at
  most L_i - 1 further additions of non-zero partial sums; adding an exact zero -- an idle lane of a lane group, a padding
  entry -- rounds nothing; 2 more for slack in the first-order expansion);
* the matrix generator of the route tests.
"""
import numpy as np

# ---------------------------------------------------------------------------------------------------- constants
KC = 16               # right-hand sides per chunk: one 128-byte line per staged row of X
XLD = 18              # LDS row stride (doubles) of the unpadded kernel's staged rows
NG_MAX = 10           # gather loads per thread and chunk at most: 32 * 10 = 320 distinct columns per tile
NG_SMALL = 7          # ... and 7 for tiles of up to 224
ECAP_MAX = 8192       # entries of a tile at most
LDS_BUDGET = 52 * 1024          # three workgroups per CU; the padded image may take 1 KB more
SPMV_ROWS, SPMV_CAP = 64, 2304
PLAIN, TILES, PAD = 0, 1, 2


def tile_lds_bytes(R, ucap, ecap):
    """csr_spmm_tiles: X rows [ucap][18] doubles, values [ecap] doubles, indices [ecap] u16, columns [ucap] i32, row offsets [R + 1] i32."""
    return ucap * XLD * 8 + ecap * 8 + ecap * 2 + ucap * 4 + (R + 1) * 4 + 16


def tile_pad_lds_bytes(R, ucap, ecap_pad):
    """csr_spmm_tiles_pad: X rows [ucap][16] (swizzled), values [ecap_pad + 2 R] (row r skewed by 2 r), indices, columns, two offset lists."""
    return ucap * KC * 8 + (ecap_pad + 2 * R) * 8 + ecap_pad * 2 + ucap * 4 + (2 * R + 2) * 4 + 16


def _round_up(v, m, least):
    return max(least, (v + m - 1) // m * m)


def plan(n_rows, rowptr, colidx):
    """The tile plan: the tallest R in (64, 32, 16) all of whose tiles have at most 320 distinct columns and 8192 entries and
    whose unpadded LDS image fits 52 KB.  Returns a dict; `why[R]` says what ruled a taller R out."""
    rowptr = np.asarray(rowptr, np.int64)
    colidx = np.asarray(colidx, np.int64)
    lens = np.diff(rowptr)
    out = {"state": -1, "R": 0, "ucap": 0, "ecap": 0, "ecap_pad": 0, "umax": 0, "tiles": 0, "why": {}}
    for R in (64, 32, 16):
        T = (n_rows + R - 1) // R
        uniq, umax, emax, pmax = [], 0, 0, 0
        for t in range(T):
            r0, r1 = t * R, min(n_rows, (t + 1) * R)
            u = np.unique(colidx[rowptr[r0]:rowptr[r1]])
            uniq.append(u)
            umax, emax = max(umax, len(u)), max(emax, int(rowptr[r1] - rowptr[r0]))
            pmax = max(pmax, int(((lens[r0:r1] + 7) // 8 * 8).sum()))
        if umax > 32 * NG_MAX:
            out["why"][R] = "columns"
            continue
        if emax > ECAP_MAX:
            out["why"][R] = "entries"
            continue
        ucap, ecap = _round_up(umax, 32, 32), _round_up(emax, 256, 256)
        if tile_lds_bytes(R, ucap, ecap) > LDS_BUDGET:
            out["why"][R] = "lds"
            continue
        ecap_pad = _round_up(pmax, 64, 64)
        if tile_pad_lds_bytes(R, (umax + 7) // 8 * 8, ecap_pad) > LDS_BUDGET + 1024:
            ecap_pad = 0
        tile_uptr = np.concatenate([[0], np.cumsum([len(u) for u in uniq])]).astype(np.int64)
        lidx = np.zeros(max(len(colidx), 1), np.uint16)
        for t in range(T):
            a, b = rowptr[t * R], rowptr[min(n_rows, (t + 1) * R)]
            lidx[a:b] = np.searchsorted(uniq[t], colidx[a:b])
        out.update(state=1, R=R, ucap=ucap, ecap=ecap, ecap_pad=ecap_pad, umax=umax, tiles=T, tile_uptr=tile_uptr,
                   ucols=np.concatenate(uniq).astype(np.int32) if T else np.zeros(0, np.int32), lidx=lidx[:len(colidx)])
        return out
    return out


def rows_route(pl, n_cols, k, ldx, ldy, x_aligned=True, y_aligned=True, x_stride=0, y_stride=0, no_pad=False):
    """(kind, NG) of one node-major call.  The tiled kernels move 16-byte pieces and keep a row's offset in 32 bits of 16-byte
    units: k, both ld and both batch strides even, both bases 16-byte aligned, n_cols * ldx below 2^32."""
    ok = (k % 2 == 0 and ldx % 2 == 0 and ldy % 2 == 0 and x_aligned and y_aligned and x_stride % 2 == 0 and y_stride % 2 == 0
          and n_cols * ldx < 2 ** 32)
    if pl["state"] != 1 or not ok:
        return (PLAIN, 0)
    return (PAD if pl["ecap_pad"] > 0 and not no_pad else TILES, NG_SMALL if pl["ucap"] <= 32 * NG_SMALL else NG_MAX)


def spmv_tiles_ok(n_rows, rowptr):
    rowptr = np.asarray(rowptr, np.int64)
    edges = np.append(np.arange(0, n_rows, SPMV_ROWS), n_rows)
    return bool(np.all(np.diff(rowptr[edges]) <= SPMV_CAP))


def cols_route(nnz, n_rows, k, tiles_ok):
    """0: csr_spmv_tiles (one right-hand side and every 64-row tile within 2304 entries), else the lane group by entries per row."""
    if k == 1 and tiles_ok:
        return 0
    avg = nnz / n_rows
    return 64 if avg > 40 else 32 if avg > 20 else 16 if avg > 10 else 8


# ---------------------------------------------------------------------------------------------------- matrices
class Csr:
    """A CSR matrix as raw arrays (a row may list a column twice: SciPy would merge that, the kernels do not)."""

    def __init__(self, n_rows, n_cols, rowptr, colidx, vals):
        self.shape = (n_rows, n_cols)
        self.rowptr, self.colidx, self.vals = np.asarray(rowptr, np.int64), np.asarray(colidx, np.int64), np.asarray(vals, np.float64)
        self.nnz = len(self.colidx)

    def rows(self):
        return np.repeat(np.arange(self.shape[0]), np.diff(self.rowptr))

    def unreferenced(self):
        m = np.ones(self.shape[1], bool)
        m[self.colidx] = False
        return m


def generate(n_rows, width, per, seed=0, empty=(5, 99), lengths=None, replace=False):
    """Row i draws `per` (or lengths[i % len(lengths)]) distinct columns uniformly from `width` columns, ascending; the rows in
    `empty` stay empty; values are standard normal.  replace=True draws with replacement (columns repeat within a row)."""
    rng = np.random.default_rng(seed)
    cols, rp = [], [0]
    for i in range(n_rows):
        L = per if lengths is None else int(lengths[i % len(lengths)])
        if i in empty:
            L = 0
        c = np.sort(rng.integers(0, width, L) if replace else rng.choice(width, L, replace=False))
        cols.append(c)
        rp.append(rp[-1] + L)
    colidx = np.concatenate(cols).astype(np.int64) if cols else np.zeros(0, np.int64)
    return Csr(n_rows, width, rp, colidx, rng.standard_normal(len(colidx)))


def tridiagonal(n):
    rp = np.concatenate([[0], np.cumsum(np.where((np.arange(n) == 0) | (np.arange(n) == n - 1), 2, 3))]).astype(np.int64)
    i = np.arange(n)
    c = np.stack([i - 1, i, i + 1], 1).ravel()
    keep = (c >= 0) & (c < n)
    v = np.tile([1.0, -2.5, 1.0], n)[keep] * (1.0 + 0.001 * (np.arange(keep.sum()) % 97))
    return Csr(n, n, rp, c[keep], v)


# the padded-kernel table of the route tests: (R, NG) -> (width, per); 100 rows, rows 5 and 99 empty, seed 0
TABLE = {(64, 7): (96, 5), (64, 10): (300, 8), (32, 7): (700, 8), (32, 10): (300, 17), (16, 7): (400, 17), (16, 10): (300, 33)}
UNPADDED_64_7 = (96, 57)         # ecap 3840: the padded image is 55 KB
NO_PLAN = (300, 57)              # 16-row tiles beyond the unpadded image
ROW_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 24, 31)


# ---------------------------------------------------------------------------------------------------- reference
def reference(A, X, f32=False, vals=None):
    """Y = A X in longdouble and the row-wise bound.  X: (n_cols, k) float64 (non-finite rows are fine where no entry reads
    them).  Returns (Y, bound), both (n_rows, k) longdouble."""
    v = A.vals if vals is None else np.asarray(vals, np.float64)
    if f32:
        v = v.astype(np.float32).astype(np.float64)
    X = np.asarray(X, np.float64)
    if X.ndim == 1:
        X = X[:, None]
    prod = v.astype(np.longdouble)[:, None] * X[A.colidx].astype(np.longdouble)
    Y = np.zeros((A.shape[0], X.shape[1]), np.longdouble)
    S = np.zeros_like(Y)
    r = A.rows()
    np.add.at(Y, r, prod)
    np.add.at(S, r, np.abs(prod))
    L = np.diff(A.rowptr).astype(np.longdouble)[:, None]
    return Y, (L + 2) * np.longdouble(2.0) ** -53 * S


def check(Yhat, A, X, f32=False, vals=None, what=""):
    """Every cell finite and within the row-wise bound; returns the largest error / bound ratio (printed by the callers)."""
    Y, bound = reference(A, X, f32, vals)
    Yhat = np.asarray(Yhat, np.float64).reshape(Y.shape)
    assert np.all(np.isfinite(Yhat)), f"{what}: non-finite cells at {np.argwhere(~np.isfinite(Yhat))[:4].tolist()}"
    err = np.abs(Yhat.astype(np.longdouble) - Y)
    bad = np.argwhere(err > bound)
    assert len(bad) == 0, f"{what}: {len(bad)} cells beyond the bound, first (row, rhs) {bad[:4].tolist()}, err {err[tuple(bad[0])]}, bound {bound[tuple(bad[0])]}"
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, err / bound, 0)
    return float(ratio.max()) if ratio.size else 0.0
