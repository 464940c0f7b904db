"""The Takahashi recurrence behind the exact variances and the selected inverse (csrc/gmrf_hip.hip: var_exact, selinv_pattern,
tk_coupled_y, tk_xty, tw_var_exact) on the coupling-window geometries of tests/bxt_ref.py: the cases, their well-conditioned
matrices, two longdouble references, a float64 restatement of the kernels' products with planted defects, and the checks that
turn a call's outputs into ratios.

Reference A: the recurrence on the factor the handle holds (X_i = BLOCK_LINV, C_i = BLOCK_C), in longdouble,
    Sigma_NN = X^T X,   Sigma_{i+1,i} = -Sigma_{i+1,i+1} C X,   Sigma_ii = X^T (I + C^T Sigma_{i+1,i+1} C) X,
and beside it an entrywise first-order bound of what float64 products in any order may give:
    P_N = |X|^T |X|,   P_i = |X|^T (I + |C|^T |Sigma_{i+1,i+1}| |C|) |X|,   Pc_i = |Sigma_{i+1,i+1}| |C| |X|
    E_N = g P_N,       E_i = g P_i + |X|^T |C|^T E_{i+1} |C| |X|,           Ec_i = g Pc_i + E_{i+1} |C| |X|
    g = k u / (1 - k u),  u = 2^-53,  k = 2 rmax + (bsp - cmin) + bsp + 4
k is the sum of the K lengths of the four chained products T1 = S' C_w (rmax), M = T1^T C_w (rmax), Y = (I + M) X (bsp - cmin)
and X^T Y (bsp), plus the addend and the mirror.  Every summation order of fused multiply-adds meets it, so it holds for
var_exact and for selinv_pattern, which round their chains independently.  Where the bound is zero the value is exactly zero.
It measures the recurrence alone: the factor's own error is in X and C on both sides.

Reference B: Q^-1 in longdouble (a float64 inverse and one Newton step with the residual in longdouble), errors on the
correlation scale |got_rc - Sigma_rc| / sqrt(Sigma_rr Sigma_cc) as tests/selinv_oracle.py measures them.

Both references are kept on a seeded row set of every block (all columns of those rows) and on the whole diagonal."""
import numpy as np
import scipy.sparse as sp

from tests import bxt_ref as R
from tests.potrf_ref import LONGDOUBLE_OK, SLACK

LD = np.longdouble
U = 2.0 ** -53
EPS = 2.0 ** -52
COND_CAP = 64.0
TRUTH_FACTOR = 4.0                # the kernels' gate on Reference B, in units of cond * 2^-52 (the restatement's own: 1)
REGIONS = ("diagonal below rmax", "diagonal at or above rmax", "lower tiles", "mirrored upper tiles", "coupling block")

# ------------------------------------------------------------------------------------------------ cases
BXT_CASES = ("band", "window", "ragged", "padded64", "padded100", "greedy", "lds1536")
NEW_CASES = ("late", "tiny", "split512", "window1", "window2", "window5", "window5rev")
CASES = BXT_CASES + NEW_CASES
TWISTED_CASES = ("window2", "window5", "window5rev")

# (bs, bsp, N, cmin, rmax, kst): what every case is there for
GEOMETRY = {
    "band": (128, 128, 3, 0, 128, [0, 0]),
    "window": (256, 256, 3, 64, 128, [0, 128, 192, 192]),
    "ragged": (320, 512, 3, 192, 320, [0, 0, 0, 64, 64, 320, 320, 320]),
    "padded64": (100, 128, 3, 0, 64, [0, 128]),
    "padded100": (100, 128, 3, 0, 128, [0, 0]),
    "greedy": (192, 256, 3, 0, 192, [0, 0, 0, 256]),
    "lds1536": (256, 256, 3, 0, 256, [0, 0, 64, 128]),
    "late": (256, 256, 3, 192, 64, [0, 64, 64, 64]),
    "tiny": (40, 64, 3, 0, 64, [0]),
    "split512": (512, 512, 3, 256, 192, [0, 64, 128, 256, 256, 256, 256, 256]),
    "window1": (256, 256, 1, 0, 64, [0, 256, 256, 256]),
    "window2": (256, 256, 2, 64, 128, [0, 128, 192, 192]),
    "window5": (256, 256, 5, 64, 128, [0, 128, 192, 192]),
    "window5rev": (256, 256, 5, 128, 192, [0, 64, 64, 128]),
}


def _late():
    """bs 256: rows < 64, columns >= 192, so cmin = 192 > rmax = 64 (the two-node-row elliptic shape)."""
    lo1 = [(r, 192 + r) for r in range(64)] + [(r, 255 - r // 2) for r in range(64)]
    lo2 = [(r, 192 + (r + 5) % 64) for r in range(64)] + [(r, 200 + (3 * r) % 50) for r in range(0, 64, 2)]
    return R.Pattern(256, [None, lo1, lo2], name="late")


def _tiny():
    """bs 40 (bsp 64): a single tile."""
    lo1 = [(r, c) for r in range(40) for c in (r, (r + 9) % 40)]
    lo2 = [(r, c) for r in range(40) for c in (r - 1, (r + 17) % 40) if c >= 0]
    return R.Pattern(40, [None, lo1, lo2], name="tiny")


def _split512():
    """bs 512: coupling columns >= 256 (a batch keeps the block inverses split at p = 256), rows < 192, row tile t starting
    at column 256 + 64 t."""
    def blk(o):
        e = []
        for r in range(192):
            t, q = r // 64, r % 64
            first = 256 + 64 * t
            e += [(r, first + (q + o) % 64), (r, first + 64 + (2 * q + o) % 64), (r, 511 - (q + 3 * o) % 100)]
        return e
    return R.Pattern(512, [None, blk(0), blk(1)], name="split512")


def _window_chain(N, reverse=False):
    """The window case's two lower blocks in turn; reversed: blocks and in-block indices run backwards, entry (r, c) of the
    block between i - 1 and i becomes (bs - 1 - c, bs - 1 - r) of the one between N - i and N - i + 1."""
    w = R.case("window")
    lower = [None] + [w.lower[1 + (i - 1) % 2] for i in range(1, N)]
    if reverse:
        lower = [None] + [[(255 - int(c), 255 - int(r)) for r, c in lower[N - i]] for i in range(1, N)]
    return R.Pattern(256, lower, N=N, name=f"window{N}" + ("rev" if reverse else ""))


_NEW = {"late": _late, "tiny": _tiny, "split512": _split512, "window1": lambda: _window_chain(1), "window2": lambda: _window_chain(2),
        "window5": lambda: _window_chain(5), "window5rev": lambda: _window_chain(5, True)}
_PATS, _GEOS, _MATS, _TRUTH = {}, {}, {}, {}


def pattern(name):
    if name in BXT_CASES:
        return R.case(name)
    if name not in _PATS:
        _PATS[name] = _NEW[name]()
    return _PATS[name]


class Geometry:
    """A case's sizes and window in block coordinates (rme = the rows of a coupling block that exist: min(rmax, bs))."""

    def __init__(self, name):
        pat = pattern(name)
        P = R.plan(pat, True)
        self.name, self.pat = name, pat
        self.bs, self.bsp, self.N, self.n = pat.bs, pat.bsp, pat.N, pat.n
        self.cmin, self.rmax, self.kst = int(P["cmin"]), int(P["rmax"]), [int(v) for v in P["kst"]]
        self.rme = min(self.rmax, self.bs)
        self.k = 2 * self.rmax + (self.bsp - self.cmin) + self.bsp + 4
        self.gamma = self.k * U / (1.0 - self.k * U)
        nct, nrt = (self.bsp - self.cmin) // 64, self.rmax // 64
        # as set_layout derives them: column tile u of the stored window ends at row mend[u]; column tile u of X[cmin:, :]
        # has its first non-zero row at kbx[u]
        self.mend = [max([64 * (t + 1) for t in range(nrt) if self.kst[t] <= 64 * u], default=0) for u in range(nct)]
        self.kbx = [max(0, 64 * u - self.cmin) for u in range(self.bsp // 64)]

    def summary(self):
        return (self.bs, self.bsp, self.N, self.cmin, self.rmax, self.kst)

    def window_mask(self):
        """[rme][bs - cmin]: True right of the staircase, where a coupling block may hold a non-zero."""
        rows = np.arange(self.rme)
        return np.arange(self.bs - self.cmin)[None, :] >= np.array(self.kst)[rows // 64][:, None]

    def rows(self, i):
        """The checked rows of block i: 0, 63, 64, rmax - 1, rmax, bs - 1 where they exist and 16 seeded ones, dealt out over
        the 64-row tiles in turn so that every row tile has one."""
        fixed = [r for r in (0, 63, 64, self.rmax - 1, self.rmax, self.bs - 1) if 0 <= r < self.bs]
        rng = np.random.default_rng([77, self.bs, self.rmax, i])
        nt = (self.bs + 63) // 64
        seeded = [64 * (j % nt) + int(rng.integers(0, min(64, self.bs - 64 * (j % nt)))) for j in range(16)]
        return np.unique(np.array(fixed + seeded, np.int64))


def geometry(name):
    if name not in _GEOS:
        _GEOS[name] = Geometry(name)
    return _GEOS[name]


# ------------------------------------------------------------------------------------------------ values
def spd_matrix(pat, p):
    """Problem p on a pattern: pat.values(p) on the strict lower triangle, symmetrised, every diagonal entry 1 + the absolute
    sum of its row (so cond_2 stays small and the recurrence's own rounding is what a test sees).  Sorted CSC."""
    v = pat.values(p)
    low = pat.rowval > pat.colidx
    L = sp.coo_matrix((v[low], (pat.rowval[low], pat.colidx[low])), shape=(pat.n, pat.n)).tocsc()
    A = L + L.T
    d = 1.0 + np.asarray(abs(A).sum(axis=1)).ravel()
    Q = sp.csc_matrix(A + sp.diags(d))
    Q.sort_indices()
    return Q


def matrix(name, p):
    """(Q, cond_2) of problem p of a case: built once, left unchanged."""
    key = (name, p)
    if key not in _MATS:
        Q = spd_matrix(pattern(name), p)
        ev = np.linalg.eigvalsh(Q.toarray())
        _MATS[key] = (Q, float(ev[-1] / ev[0]))
    return _MATS[key]


# ------------------------------------------------------------------------------------------------ the pattern asked for
class SelPattern:
    """The dense diagonal blocks plus Sigma_{i+1,i}[0:rme, :] in both triangles, as a CSR pattern: row r of block i holds all
    of block i - 1's columns (r < rme), all of its own block's, and the first rme columns of block i + 1."""

    def __init__(self, geo):
        self.geo = geo
        bs, N, rme = geo.bs, geo.N, geo.rme
        blk = np.repeat(np.arange(N), bs)
        loc = np.tile(np.arange(bs), N)
        prev = np.where((blk > 0) & (loc < rme), bs, 0)
        nxt = np.where(blk < N - 1, rme, 0)
        self.own = prev.astype(np.int64)                       # offset of the row's own block in its row
        self.indptr = np.concatenate([[0], np.cumsum(prev + bs + nxt)]).astype(np.int64)
        self.nnz = int(self.indptr[-1])
        idx = np.empty(self.nnz, np.int32)
        for g in range(geo.n):
            i, a = int(blk[g]), int(self.indptr[g])
            if prev[g]:
                idx[a:a + bs] = np.arange((i - 1) * bs, i * bs)
                a += bs
            idx[a:a + bs] = np.arange(i * bs, (i + 1) * bs)
            if nxt[g]:
                idx[a + bs:a + bs + rme] = np.arange((i + 1) * bs, (i + 1) * bs + rme)
        self.indices = idx

    def csr(self):
        return sp.csr_matrix((np.ones(self.nnz), self.indices, self.indptr), shape=(self.geo.n, self.geo.n))

    def pos(self, gr, gc):
        """The slot of entry (gr, gc) (global indices, arrays broadcast); it must lie in the pattern."""
        gr, gc = np.broadcast_arrays(np.asarray(gr, np.int64), np.asarray(gc, np.int64))
        bs, rme = self.geo.bs, self.geo.rme
        bi, bj, r, c = gr // bs, gc // bs, gr % bs, gc % bs
        assert (np.abs(bi - bj) <= 1).all() and (r[bj < bi] < rme).all() and (c[bj > bi] < rme).all()
        off = np.where(bj < bi, c, np.where(bj == bi, self.own[gr] + c, self.own[gr] + bs + c))
        return self.indptr[gr] + off

    def diag_rows(self, vals, i, rows):
        bs = self.geo.bs
        return vals[self.pos(i * bs + rows[:, None], i * bs + np.arange(bs)[None, :])]

    def low_rows(self, vals, i, rows):
        """Sigma_{i+1,i}[rows, :] from the lower triangle's slots and from the upper one's."""
        bs = self.geo.bs
        gr, gc = (i + 1) * bs + rows[:, None], i * bs + np.arange(bs)[None, :]
        return vals[self.pos(gr, gc)], vals[self.pos(gc, gr)]

    def fill(self, diag, low):
        """The values array of full blocks diag[i] (bs x bs) and low[i] (rme x bs): what a call on this pattern returns."""
        bs, rme, N = self.geo.bs, self.geo.rme, self.geo.N
        vals = np.full(self.nnz, np.nan)
        a = np.arange(bs)
        for i in range(N):
            vals[self.pos(i * bs + a[:, None], i * bs + a[None, :])] = diag[i]
            if i < N - 1:
                gr, gc = (i + 1) * bs + np.arange(rme)[:, None], i * bs + a[None, :]
                vals[self.pos(gr, gc)] = low[i]
                vals[self.pos(gc, gr)] = low[i]
        assert not np.isnan(vals).any()
        return vals


_SELPATS = {}


def sel_pattern(name):
    if name not in _SELPATS:
        _SELPATS[name] = SelPattern(geometry(name))
    return _SELPATS[name]


# ------------------------------------------------------------------------------------------------ Reference A
def clean_factor(geo, Xs, Cs):
    """What the recurrence may read of the blocks a handle returns: X_i's lower triangle, and of C_i the stored window's
    cells right of the staircase (the cells left of it are structural zeros that no launch writes or reads)."""
    Xc = [np.tril(np.asarray(X, np.float64)) for X in Xs]
    Cc = []
    for C in Cs:
        W = np.zeros((geo.rme, geo.bs - geo.cmin))
        W[geo.window_mask()] = np.asarray(C, np.float64)[:geo.rme, geo.cmin:][geo.window_mask()]
        Cc.append(W)
    return Xc, Cc


def _times_lower(A, Xw, cm):
    """A @ Xw for Xw = X[cm:, :] of a lower-triangular X: the rows of column tile c0 above c0 - cm are zero."""
    out = np.empty((A.shape[0], Xw.shape[1]), LD)
    for c0 in range(0, Xw.shape[1], 64):
        k0 = max(0, c0 - cm)
        out[:, c0:c0 + 64] = A[:, k0:] @ Xw[k0:, c0:c0 + 64]
    return out


def _symmetric_product(A, Bm, m, a_lower=False):
    """(A^T Bm)[0:m, 0:m] where it is symmetric: its lower row tiles, mirrored (a_lower: A is lower triangular, the rows of
    its column tile r0 above r0 are zero)."""
    out = np.zeros((m, m), LD)
    for r0 in range(0, m, 64):
        r1 = min(r0 + 64, m)
        k0 = r0 if a_lower else 0
        out[r0:r1, :r1] = A[k0:, r0:r1].T @ Bm[k0:, :r1]
    return np.tril(out) + np.tril(out, -1).T


class ReferenceA:
    """rows[i]; d_val / d_bnd[i]: Sigma_ii[rows, :] and its bound; l_rows[i] = the rows below rme, l_val / l_bnd[i]:
    Sigma_{i+1,i}[l_rows, :]; v_val / v_bnd[i]: the diagonal of Sigma_ii."""

    def __init__(self, geo, Xs, Cs):
        N, cm, rme = geo.N, geo.cmin, geo.rme
        Xc, Cc = clean_factor(geo, Xs, Cs)
        g = geo.gamma * (1.0 if LONGDOUBLE_OK else 2.0)        # (a reference in float64 has the same error itself)
        self.geo = geo
        self.rows = [geo.rows(i) for i in range(N)]
        self.d_val, self.d_bnd, self.v_val, self.v_bnd = [None] * N, [None] * N, [None] * N, [None] * N
        self.l_rows, self.l_val, self.l_bnd = [None] * N, [None] * N, [None] * N
        S = E = None                                           # the leading rme x rme block of Sigma_{i+1,i+1}, its bound
        for i in range(N - 1, -1, -1):
            X = Xc[i].astype(LD)
            aX = np.abs(Xc[i])
            Y, PY, EY = X.copy(), aX.copy(), np.zeros_like(aX)
            rows = self.rows[i]
            if i < N - 1:
                C = Cc[i].astype(LD)
                aC, aS = np.abs(Cc[i]), np.abs(S).astype(np.float64)
                T1 = S @ C
                Y[cm:] += _times_lower(_symmetric_product(C, T1, C.shape[1]), X[cm:], cm)
                PY[cm:] += (aC.T @ (aS @ aC)) @ aX[cm:]
                EY[cm:] = (aC.T @ (E @ aC)) @ aX[cm:]
                lr = rows[rows < rme]
                self.l_rows[i] = lr
                self.l_val[i] = -_times_lower(T1[lr], X[cm:], cm)
                self.l_bnd[i] = (g * ((aS @ aC) @ aX[cm:]) + (E @ aC) @ aX[cm:])[lr] * SLACK
            bound = (g * (aX.T @ PY) + aX.T @ EY) * SLACK
            self.d_val[i] = X[:, rows].T @ Y
            self.d_bnd[i] = bound[rows]
            self.v_val[i] = (X * Y).sum(axis=0)
            self.v_bnd[i] = np.diag(bound).copy()
            if i > 0:
                S = _symmetric_product(X, Y, rme, a_lower=True)
                E = bound[:rme, :rme]


def _ratios(got, val, bnd):
    """|got - val| / bnd entrywise; where the bound is zero the value must be exactly zero (else infinite); NaN is infinite."""
    err = np.abs(got.astype(LD) - val).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0.0, 0.0, err / bnd)
    q[np.isnan(q)] = np.inf
    return q


def _region_of(geo, r, c):
    if r == c:
        return REGIONS[0] if r < geo.rmax else REGIONS[1]
    return REGIONS[2] if r > c else REGIONS[3]


def check_selinv(ref, selpat, vals):
    """One problem's selected inverse on sel_pattern against Reference A: (worst ratio, where it occurs, ratio by region);
    where = (step, region, row, column) in block coordinates.  A ratio <= 1 passes."""
    geo = ref.geo
    worst, where = 0.0, None
    by_region = dict.fromkeys(REGIONS, 0.0)
    a = np.arange(geo.bs)
    for i in range(geo.N):
        rows = ref.rows[i]
        q = _ratios(selpat.diag_rows(vals, i, rows), ref.d_val[i], ref.d_bnd[i])
        kinds = np.where(rows[:, None] == a[None, :], np.where(rows[:, None] < geo.rmax, 0, 1), np.where(rows[:, None] > a[None, :], 2, 3))
        for k in range(4):
            if (kinds == k).any():
                by_region[REGIONS[k]] = max(by_region[REGIONS[k]], float(q[kinds == k].max()))
        if q.max() > worst:
            j = np.unravel_index(np.argmax(q), q.shape)
            worst, where = float(q.max()), (i, _region_of(geo, int(rows[j[0]]), int(j[1])), int(rows[j[0]]), int(j[1]))
        if i < geo.N - 1 and len(ref.l_rows[i]):
            lr = ref.l_rows[i]
            for got in selpat.low_rows(vals, i, lr):
                q = _ratios(got, ref.l_val[i], ref.l_bnd[i])
                by_region[REGIONS[4]] = max(by_region[REGIONS[4]], float(q.max()))
                if q.max() > worst:
                    j = np.unravel_index(np.argmax(q), q.shape)
                    worst, where = float(q.max()), (i, REGIONS[4], int(lr[j[0]]), int(j[1]))
    return worst, where, by_region


def check_var(ref, var):
    """One problem's exact variances (n values) against Reference A's diagonal: (worst ratio, (step, region, index))."""
    geo = ref.geo
    worst, where = 0.0, None
    for i in range(geo.N):
        q = _ratios(np.asarray(var[i * geo.bs:(i + 1) * geo.bs]), ref.v_val[i], ref.v_bnd[i])
        if q.max() > worst:
            j = int(np.argmax(q))
            worst, where = float(q.max()), (i, _region_of(geo, j, j), j)
    return worst, where


# ------------------------------------------------------------------------------------------------ Reference B
class Truth:
    """Sigma = Q^-1 of one problem in longdouble, kept where Reference A is: diag (n), d_val[i] = Sigma_ii[rows, :],
    l_val[i] = Sigma_{i+1,i}[l_rows, :]; resid = max |I - Q Sigma|."""

    def __init__(self, geo, Q, cond):
        n, bs, N, rme = geo.n, geo.bs, geo.N, geo.rme
        self.geo, self.cond = geo, cond
        Qc = sp.csr_matrix(Q)
        S0 = np.linalg.inv(Qc.toarray())

        def residual(S):
            """I - Q S in longdouble, one stored entry of Q at a time."""
            Rm = np.eye(n, dtype=LD)
            rr = np.repeat(np.arange(n), np.diff(Qc.indptr))
            k_in_row = np.arange(Qc.nnz) - Qc.indptr[rr]
            for k in range(int(k_in_row.max()) + 1):           # the k-th entry of every row that has one: distinct rows
                e = np.flatnonzero(k_in_row == k)
                Rm[rr[e]] -= Qc.data[e].astype(LD)[:, None] * S[Qc.indices[e]]
            return Rm

        S0l = S0.astype(LD)
        S1 = S0l + (S0 @ residual(S0l).astype(np.float64)).astype(LD)      # (the correction is ~ 1e-16 S0: float64 carries it)
        self.resid = float(np.abs(residual(S1)).max())
        self.diag = np.diag(S1).copy()
        self.rows = [geo.rows(i) for i in range(N)]
        self.l_rows = [self.rows[i][self.rows[i] < rme] for i in range(N)]
        self.d_val = [S1[i * bs + self.rows[i], i * bs:(i + 1) * bs] for i in range(N)]
        self.l_val = [S1[(i + 1) * bs + self.l_rows[i], i * bs:(i + 1) * bs] for i in range(N - 1)]


def truth(name, p):
    key = (name, p)
    if key not in _TRUTH:
        Q, cond = matrix(name, p)
        _TRUTH[key] = Truth(geometry(name), Q, cond)
    return _TRUTH[key]


def truth_selinv(tr, selpat, vals):
    """Largest correlation-scale error of one problem's selected inverse, in units of cond * 2^-52."""
    geo = tr.geo
    worst = 0.0
    for i in range(geo.N):
        d = np.sqrt(tr.diag[i * geo.bs:(i + 1) * geo.bs])
        rows = tr.rows[i]
        err = np.abs(selpat.diag_rows(vals, i, rows).astype(LD) - tr.d_val[i]) / (d[rows][:, None] * d[None, :])
        worst = max(worst, float(np.nan_to_num(err.astype(np.float64), nan=np.inf).max()))
        if i < geo.N - 1 and len(tr.l_rows[i]):
            dn = np.sqrt(tr.diag[(i + 1) * geo.bs:(i + 2) * geo.bs])
            for got in selpat.low_rows(vals, i, tr.l_rows[i]):
                err = np.abs(got.astype(LD) - tr.l_val[i]) / (dn[tr.l_rows[i]][:, None] * d[None, :])
                worst = max(worst, float(np.nan_to_num(err.astype(np.float64), nan=np.inf).max()))
    return worst / (tr.cond * EPS)


def truth_var(tr, var):
    """Largest |var_r - Sigma_rr| / Sigma_rr in units of cond * 2^-52."""
    err = np.abs(np.asarray(var).astype(LD) - tr.diag) / tr.diag
    return float(np.nan_to_num(err.astype(np.float64), nan=np.inf).max()) / (tr.cond * EPS)


# ------------------------------------------------------------------------------------------------ float64 restatement
DEFECTS = ("drop_t1", "drop_m", "drop_y", "drop_xty", "mend_short", "kbx_late", "mirror_skipped", "mirror_skipped_s", "diag_without_y")


def _tile_of_defect(geo):
    """The column tile of the stored window whose bounds a planted defect moves: the last one (every row tile reaches it)."""
    return (geo.bs - geo.cmin - 1) // 64


def restate(geo, Xs, Cs, defect=None):
    """The kernels' products in float64, in their order: per step T1 = S' C_w, M = T1^T C_w on its lower tiles and mirrored,
    Y[cmin:] = (I + M) X[cmin:], Sigma_{i+1,i}[0:rmax] = -T1 X[cmin:], S_ii = X^T Y on its lower tiles and mirrored; the
    variances below rmax from S_ii's diagonal, those at or above rmax (all of them in block 0) from column dots of X and Y.
    A K bound that is right skips exact zeros only, so the clean products are plain ones.  Returns (diag, low, var):
    full blocks and the variance vector.  `defect`: one of DEFECTS, planted in every step."""
    N, bs, cm, rme, rm = geo.N, geo.bs, geo.cmin, geo.rme, geo.rmax
    Xc, Cc = clean_factor(geo, Xs, Cs)
    u = _tile_of_defect(geo)
    cols = slice(64 * u, 64 * u + 64)                          # of the window
    diag, low, var = [None] * N, [None] * max(N - 1, 0), np.zeros(geo.n)
    S = None

    def lower_mirrored(A, Bm, skip=False):
        """A^T Bm formed on its lower triangle and mirrored; `skip`: the upper-right 32 x 32 quarter of the first diagonal
        tile, which the 32 x 32-tile kernel does not write, is left as it was (zero: "mirror_skipped" does it to M)."""
        Lw = np.tril(A.T @ Bm)
        out = Lw + np.tril(Lw, -1).T
        if skip:
            out[0:32, 32:64] = 0.0
        return out

    for i in range(N - 1, -1, -1):
        X = Xc[i]
        Xw = X[cm:]
        Y = X.copy()
        if i < N - 1:
            C = Cc[i]
            Cb = C.copy()                                      # C_w as the K bound mend[] lets the products see it
            if defect == "mend_short":
                Cb[geo.mend[u] - 64:geo.mend[u], cols] = 0.0
            Xb = Xw.copy()                                     # X[cmin:, :] as the K bound kbx[] lets the products see it
            if defect == "kbx_late":
                t = u + cm // 64                               # column tile of X whose first non-zero row tile is window row tile u
                Xb[geo.kbx[t]:geo.kbx[t] + 64, 64 * t:64 * t + 64] = 0.0
            Sl = S[:rme, :rme]
            T1 = Sl @ Cb
            if defect == "drop_t1":
                T1 -= Sl[:, 0:64] @ Cb[0:64]
            M = lower_mirrored(T1, Cb, skip=defect == "mirror_skipped")
            if defect == "drop_m":
                M -= lower_mirrored(T1[0:64], Cb[0:64])
            Y[cm:] = M @ Xb + Xw
            if defect == "drop_y":
                Y[cm:] -= M[:, cols] @ Xb[cols]
            low[i] = -(T1 @ Xb)
            Sii = lower_mirrored(X[:cm], X[:cm]) + lower_mirrored(Xb, Y[cm:])
            if defect == "drop_xty":
                Sii -= lower_mirrored(Xb[cols], Y[cm:][cols])
        else:
            Sii = lower_mirrored(X, X)
        diag[i] = Sii
        s = slice(i * bs, (i + 1) * bs)
        var[s] = (X * (X if defect == "diag_without_y" else Y)).sum(axis=0)
        if i > 0:
            k = min(rm, bs)
            var[s][:k] = np.diag(Sii)[:k]
        S = Sii
        if defect == "mirror_skipped_s":                       # the leading block handed to the next step, its first diagonal tile
            S = Sii.copy()
            S[0:32, 32:64] = 0.0
    return diag, low, var
