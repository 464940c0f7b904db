"""A plain NumPy statement of the in-block Cholesky (potrf_block, csrc/gmrf_hip.hip; kernels in csrc/potrf_step.hpp and
csrc/potrf_persist.hpp) for the route-level tests of gmrf_test_potrf_route: inputs, the contract of the three buffers, the
derived bounds of the factor and of the inverse, and float64 restatements of each route's arithmetic (CPU only).

Contract of the buffers, as the kernels have it (tiles are 64 x 64, (r, c) = tile row / column)
------------------------------------------------------------------------------------------------
S in     read: the tiles r >= c; of a diagonal tile the lower triangle with the diagonal.  The strict upper triangle of a diagonal
         tile is loaded with the tile but reaches no output (tile_potrf_inv: "lower triangle valid"; every in-tile operand is masked
         by row >= column).  The tiles r < c are never addressed.  build_buffers puts NaN on both.  S is overwritten (work space).
L, X in  the tiles r < c are INPUTS: they must hold zeros.  Nothing in potrf_block writes them (alloc_factor zeroes them once),
         and the triangular operands of the GEMM launches (TRI_* of gemm_f64.hpp: "the zero part inside the boundary tile must hold
         real zeros") read them wherever a kernel tile wider than 64 straddles the block diagonal -- potrf_block's own doubling
         products among them.  A finite sentinel other than zero would therefore change results; the sentinel here is -0.0: a real
         zero to every product, and a write of +0.0 or of anything else shows in its bits.  Everything else of L and X goes in as NaN.
L out    tiles r > c: L; diagonal tiles: L with an exactly zero strict upper triangle (panel_lead stores the zeros); tiles r < c
         untouched.  One exception: the split inverse with p = 256 and no kept L (`in_slot`) forms L[256:, 0:256] in X's storage
         and never writes that part of L.
X out    full inverse: like L.  Split inverse (route[2] = p > 0; a = [0, p), b = [p, bs)): X[a, a] = L[a, a]^-1,
         X[b, b] = L[b, b]^-1, and X[b, a] holds L[b, a] -- a copy, bit for bit, or on the in_slot form the only one.
info     0, or 1 + the index of a problem that met a non-positive pivot (the first writer wins).

Criteria (u = 2^-53, g(k) = k u / (1 - k u), every bound a matrix, compared element by element on the lower triangle)
-----------------------------------------------------------------------------------------------------------------------
Inverse, right residual.  Every assembly solves L X = I: substitution by columns inside a 16 x 16 block (inv16), then
  X[r, c] = -X_rr T,  T = sum_{c <= p < r} L[r, p] X[p, c]
over 16-wide blocks inside a tile, over tiles in a block of `rows_upto` columns (xrow_strip and the persistent kernel), and
X21 = -X22 (L21 X11) per doubling level, which is the same statement with two blocks.  With fl(T) = T + d1, |d1| <= g(K1) Tabs,
Tabs = sum |L[r, p]| |X[p, c]|, K1 the length of the sum; fl(X_rr fl(T)) = X_rr fl(T) + d2, |d2| <= g(K2) |X_rr| |fl(T)|; and
L_rr X_rr = I + E_rr:
  (L X)[r, c] = T + L_rr X[r, c] = -d1 - E_rr fl(T) - L_rr d2
  |L X - I|[r, c] <= Br[r, c] := g(K1) Tabs + (Br[r, r] + g(K2) |L_rr| |X_rr|) Tabs (1 + 2^-20)
(the last factor covers |fl(T)| <= (1 + g(K1)) Tabs and the second-order terms).  Base: a triangular system solved by
substitution has a backward error g(n) |L| (Higham, Accuracy and Stability of Numerical Algorithms, theorem 8.5) in any order;
the reciprocal pivots (rsq + one Halley step, then a product where the theorem divides) add four roundings:
Br = g(16 + 4) |L_II| |X_II| on the 16 x 16 diagonal blocks.
Inverse, the criterion checked:  X L - I = X (L X - I) X^-1 and X^-1 = (I + E)^-1 L with E = L X - I, so
  |X L - I| <= bound_X := |X| (Br + 2 Br Br) |L| (1 + 2^-20)            (needs ||Br||_inf <= 1/2, else the check fails)
Split form: the two diagonal blocks, each with its own L.

Factor.  R = A - L L^T.  M = |L| |L|^T.  An entry of the trailing block is updated by products summed FROM ZERO in MFMA
accumulators and subtracted once each (potrf_step, potrf_update, diag_update_*, the GEMM launches with beta = 1): a group of K
terms contributes g(K) of its part of M, a subtraction one u of a partial sum that M bounds.  Groups: 64 columns per step; the
panel routes 64 pw columns per finished panel (pw = 4 tiles: K = 256) and 64 or 128 inside the panel.  Subtractions: at most
nt - 1 outside the tile.  Inside the tile (tile_potrf_inv) an entry takes one subtraction of a sum of up to 48 terms, up to 15
fma rank-1 updates and the scaling by the reciprocal pivot (rinv to 2 u, l = a rinv, l_jj = p rinv: 6 roundings on l l^T):
  k = Kmax + (nt - 1) + 16 + 6,     |R| <= g(k) M      on the diagonal tiles, and as the update part of every other tile.
The rows below a diagonal block P are a PRODUCT with its explicit inverse, L[r, P] = fl(S'[r, P] X_P^T) = S' X_P^T + D,
|D| <= g(K_P) |S'| |X_P|^T, not a triangular solve.  With L_P X_P = I + E_P (|E_P| <= Br on P) and S' the updated block,
  S' - L[r, P] L_P^T = -S' E_P^T - D L_P^T,    |S'| <= |L[r, P]| |L_P|^T (1 + second order)
  |R|[r, P] <= g(k) M[r, P] + |L[r, P]| (g(K_P) |L_P|^T |X_P|^T |L_P|^T + |L_P|^T Br[P, P]^T) (1 + 2^-20)
P is the 64-wide tile on the step routes and inside the panels of the one-problem routes; on the 256-column panel route the tile
(persistent form) or the tile and the 128-wide block (potrf_diag128) inside a panel and the 256-wide panel below it.

Evaluation.  bs <= 256: R and X L - I in longdouble (tile by tile over the lower triangle), every element.  bs >= 512: every
element in float64 BLAS, the bound widened by that evaluation's own (n + 2) u |L| |L|^T (and (n + 2) u |X| |L|), and in
longdouble on a seeded row set with one row of every 16-row group.  Without an 80-bit longdouble every bound is widened by the
float64 term.  No constant here was fitted to a kernel's output; tests/test_potrf_ref_cpu.py holds the restatements below to
the bounds and shows that they notice a dropped MFMA step, a tile of the wrong problem, a transposed 16 x 16 block, a relative
error of 2^-36 and a tile that was not written.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import __graft_entry__

U = 2.0 ** -53
LD = np.longdouble
LONGDOUBLE_OK = bool(np.finfo(np.longdouble).eps <= 2.0 ** -63)
SLACK = 1.0 + 2.0 ** -20

ROUTE_FUSED, ROUTE_BIG_ONE, ROUTE_PANELS256, ROUTE_STEPS = 1, 2, 3, 4
ROUTE_NAMES = {1: "fused", 2: "big_one", 3: "panels256", 4: "steps"}
_SW = __graft_entry__.load_package().Switch         # (plain ints: the cases' ids and records carry numbers)
BIT_BATCH_ROUTES, BIT_FORK, BIT_DOUBLING, BIT_NO_LOOKAHEAD = int(_SW.BATCH_ROUTES), int(_SW.FORK_GRAPH), int(_SW.DOUBLING_INVERSE), int(_SW.NO_LOOKAHEAD)
BIT_NO_XSPLIT, BIT_NO_PERSIST, BIT_NO_PERSIST_PANELS = int(_SW.NO_XSPLIT), int(_SW.NO_PERSIST), int(_SW.NO_PERSIST_PANELS)
FAMILIES = ("dominant", "graded", "lattice", "spectrum")
SCALES = (1.0, 1e-3, 1e6, 1e-5, 1e2)
CUS = 256                         # compute units of the device the routes are planned for


def g(k):
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------------------------------------ inputs
_SPD = {}


def spd(family, n, seed):
    """A symmetric positive definite n x n matrix of one family (memoised, read-only)."""
    key = (family, n, seed)
    if key in _SPD:
        return _SPD[key]
    rng = np.random.default_rng([seed, n, FAMILIES.index(family)])
    if family == "dominant":
        G = rng.standard_normal((n, n))
        A = G @ G.T + n * np.eye(n)
    elif family == "graded":
        G = rng.standard_normal((n, n))
        d = 10.0 ** (-4.0 * np.arange(n) / n)
        A = d[:, None] * (G @ G.T / n + np.eye(n)) * d[None, :]
    elif family == "lattice":
        ny, nx = 8, n // 8
        idx = np.arange(n).reshape(ny, nx)
        A = (4.0 + 1e-2) * np.eye(n)
        for a, b in ((idx[:, :-1], idx[:, 1:]), (idx[:-1, :], idx[1:, :])):
            A[a.ravel(), b.ravel()] = -1.0
            A[b.ravel(), a.ravel()] = -1.0
        p = rng.permutation(n)
        A = A[p][:, p]
    elif family == "spectrum":
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        A = (Q * np.logspace(0.0, -10.0, n)) @ Q.T
    else:
        raise ValueError(family)
    A = 0.5 * (A + A.T)
    A.setflags(write=False)
    _SPD[key] = A
    return A


def problems(family, n, seed, batch):
    """The inputs of a batch: problem p takes the next family, its own seed and its own scale, so that a tile read from the
    neighbouring problem cannot pass.  [(family, n, seed, scale)]"""
    f0 = FAMILIES.index(family)
    return [(FAMILIES[(f0 + p) % len(FAMILIES)], n, seed + 17 * p, SCALES[p % len(SCALES)]) for p in range(batch)]


def matrix(prob):
    family, n, seed, scale = prob
    A = spd(family, n, seed)
    return A if scale == 1.0 else A * scale


def tile_masks(n):
    t = np.arange(n) // 64
    upper_tiles = t[:, None] < t[None, :]
    diag_upper = (t[:, None] == t[None, :]) & (np.arange(n)[:, None] < np.arange(n)[None, :])
    return upper_tiles, diag_upper


def build_buffers(mats):
    """S, L, X of a call ([batch][n][n]) as the contract has them: whatever is not an input holds NaN; the tiles above the
    block diagonal of L and X hold the sentinel -0.0."""
    n = mats[0].shape[0]
    up, du = tile_masks(n)
    S = np.stack([np.where(up | du, np.nan, A) for A in mats])
    L = np.full_like(S, np.nan)
    L[:, up] = -0.0
    return S, L, L.copy()


# ------------------------------------------------------------------------------------------------ forms
@dataclass(frozen=True)
class Form:
    """What a call does, as the host code of potrf_block decides it (potrf_route, planned_xsplit, persist_demand)."""
    n: int
    route: int
    persist: int         # gmrf_stats.persist_route the call reports
    xsplit: int
    in_slot: bool        # L[256:, 0:256] lives in X's storage only
    kmax: int            # longest group of one subtraction
    rows_upto: int       # the inverse is assembled by rows inside blocks of this size, by doubling above
    inv: str             # which explicit inverses the rows below meet: "tile", "panel_persist", "panel_diag128"

    @property
    def nt(self):
        return self.n // 64

    @property
    def k(self):
        return self.kmax + (self.nt - 1) + 16 + 6


def persist_tiles(nt, j0, j1, xrows):
    n = 0
    if xrows == 2:
        n = 1 if nt - 1 > j0 else 0
    elif xrows:
        n = nt - 1 - j0
    for c in range(j0 + 1, j1):
        n += nt - 1 - c + (1 if c >= j0 + 2 else 0)
    return n


def plan(n, batch=1, bits=0, cmin=0, keep_l=1, panel_tiles=4):
    nt = n // 64
    one = batch == 1 and not bits & BIT_BATCH_ROUTES
    if one:
        route = ROUTE_FUSED if nt <= 16 else ROUTE_BIG_ONE
    elif bits & BIT_FORK and nt >= 8:
        route = ROUTE_STEPS
    else:
        route = ROUTE_PANELS256 if nt >= 4 else ROUTE_STEPS
    no_persist = bool(bits & BIT_NO_PERSIST) or n < 128 or bool(bits & BIT_FORK)
    xsplit, in_slot, persist = 0, False, 0
    if route == ROUTE_FUSED:
        rows = n if not bits & BIT_DOUBLING else 64
        if not no_persist and not bits & (BIT_NO_LOOKAHEAD | BIT_DOUBLING) and nt >= 2 and 1 + persist_tiles(nt, 0, nt, 1) <= CUS:
            persist = 1
        return Form(n, route, persist, 0, False, 64, rows, "tile")
    if route == ROUTE_BIG_ONE:
        pw = panel_tiles if panel_tiles in (2, 8) else 4
        claim = 1 + persist_tiles(nt, 0, min(nt, 4), 0)
        if not no_persist and not bits & BIT_NO_LOOKAHEAD and claim <= CUS and 1 + persist_tiles(nt, 0, pw, 0) <= claim:
            persist = 2
        return Form(n, route, persist, 0, False, 64 * pw, 64, "tile")
    if route == ROUTE_STEPS:
        pw = (panel_tiles if panel_tiles in (2, 8) else 4) if nt >= 8 else nt
        return Form(n, route, 0, 0, False, 64 * min(pw, nt), 64, "tile")
    if not bits & BIT_NO_XSPLIT and nt >= 8 and cmin >= 256:
        p = 256
        while 2 * p <= cmin:
            p *= 2
        if p < n:
            xsplit, in_slot = p, (p == 256 and not keep_l)
    if not no_persist and not bits & BIT_NO_PERSIST_PANELS and 7 * batch <= CUS:
        return Form(n, route, 3, xsplit, in_slot, 256, 256, "panel_persist")
    return Form(n, route, 0, xsplit, in_slot, 256, 64, "panel_diag128")


def inverse_blocks(form):
    """[(r0, r1, a, b)]: the rows [r0, r1) of the columns [a, b) are a product with the explicit inverse of L[a:b, a:b]."""
    n, out = form.n, []
    if form.inv == "tile":
        return [(a + 64, n, a, a + 64) for a in range(0, n - 64, 64)]
    for p0 in range(0, n, 256):
        if form.inv == "panel_persist":
            out += [(a + 64, p0 + 256, a, a + 64) for a in range(p0, p0 + 192, 64)]
        else:
            out += [(p0 + 64, p0 + 128, p0, p0 + 64), (p0 + 192, p0 + 256, p0 + 128, p0 + 192), (p0 + 128, p0 + 256, p0, p0 + 128)]
        if p0 + 256 < n:
            out.append((p0 + 256, n, p0, p0 + 256))
    return out


# ------------------------------------------------------------------------------------------------ bounds
def _rows_level(aL, aX, Br, lo, hi, b):
    """Block rows of b inside [lo, hi): Br of the blocks left of the diagonal from the diagonal blocks' own."""
    for r0 in range(lo + b, hi, b):
        r1 = r0 + b
        tabs = aL[r0:r1, lo:r0] @ aX[lo:r0, lo:r0]
        Br[r0:r1, lo:r0] = g(r0 - lo) * tabs + ((Br[r0:r1, r0:r1] + g(b) * (aL[r0:r1, r0:r1] @ aX[r0:r1, r0:r1])) @ tabs) * SLACK


def right_bound(aL, aX, rows_upto):
    """Br >= |L X - I| for the assembly: 16-wide blocks by substitution, rows inside tiles, rows of tiles inside blocks of
    `rows_upto`, doubling above.  aL, aX: |L|, |X| (lower triangular, full inverse layout)."""
    n = aL.shape[0]
    Br = np.zeros((n, n))
    for t in range(0, n, 64):
        for i in range(t, t + 64, 16):
            Br[i:i + 16, i:i + 16] = g(16 + 4) * (aL[i:i + 16, i:i + 16] @ aX[i:i + 16, i:i + 16])
        _rows_level(aL, aX, Br, t, t + 64, 16)
    if rows_upto > 64:
        for t in range(0, n, rows_upto):
            _rows_level(aL, aX, Br, t, t + rows_upto, 64)
    hh = rows_upto
    while hh < n:
        for t in range(0, n, 2 * hh):
            _rows_level(aL, aX, Br, t, t + 2 * hh, hh)
        hh *= 2
    return Br


def clean(form, L, X):
    """(L, X) of one problem as lower triangular matrices in the full layout: the tiles above the block diagonal and the strict
    upper triangles dropped, the split form's L block taken out of X (and, in_slot, into L).  Copies."""
    p = form.xsplit
    Lc, Xc = np.tril(L), np.tril(X)
    if p:
        if form.in_slot:
            Lc[p:, :p] = X[p:, :p]
        Xc[p:, :p] = 0.0
    return Lc, Xc


def bounds(form, Lc, Xc):
    """(bound_L, bound_X, M, XLabs): the two criteria's bounds and the magnitude products the float64 evaluations are
    charged with; None where ||Br||_inf > 1/2 (outputs no first-order bound applies to: check fails them).  bound_X is block
    diagonal on the split form."""
    n = form.n
    aL, aX = np.abs(Lc), np.abs(Xc)
    Br = right_bound(aL, aX, form.rows_upto)
    if not np.max(Br.sum(axis=1)) <= 0.5:           # the first-order bounds do not apply: L and X are not a factor and its inverse
        return None
    M = aL @ aL.T
    bL = g(form.k) * M
    for r0, r1, a, b in inverse_blocks(form):
        Lp, Xp = aL[a:b, a:b], aX[a:b, a:b]
        bL[r0:r1, a:b] += (aL[r0:r1, a:b] @ (g(b - a) * (Lp.T @ (Xp.T @ Lp.T)) + Lp.T @ Br[a:b, a:b].T)) * SLACK
    XLabs = aX @ aL
    p = form.xsplit
    E = Br + 2.0 * (Br @ Br)
    if p:
        bX = np.zeros((n, n))
        for s in (slice(0, p), slice(p, n)):
            bX[s, s] = (aX[s, s] @ E[s, s]) @ aL[s, s] * SLACK
    else:
        bX = (aX @ E) @ aL * SLACK
    return bL, bX, M, XLabs


def row_set(n, seed=0):
    """One row of every 16-row group (so of every tile row and of every MFMA row group), seeded."""
    rng = np.random.default_rng([seed, n, 16])
    return np.arange(0, n, 16) + rng.integers(0, 16, n // 16)


def _ld_lower_products(P, Q, rows=None):
    """tril(P @ Q^T) (P, Q lower triangular) in longdouble: tile by tile over the lower triangle, or the given rows only."""
    n = P.shape[0]
    Pl, Ql = P.astype(LD), Q.astype(LD)
    if rows is not None:
        out = np.zeros((len(rows), n), LD)
        for i, r in enumerate(rows):
            out[i, :r + 1] = Ql[:r + 1, :r + 1] @ Pl[r, :r + 1]
        return out
    out = np.zeros((n, n), LD)
    for r0 in range(0, n, 64):
        out[r0:r0 + 64, :r0 + 64] = Pl[r0:r0 + 64, :r0 + 64] @ Ql[:r0 + 64, :r0 + 64].T
    return out


def _ratio(err, bound):
    """Largest err / bound (the caller has zeroed what lies outside the lower triangle); a NaN anywhere, or an error where the
    bound is zero, is infinite."""
    e = np.asarray(err, dtype=np.float64)
    if np.isnan(e).any() or np.isnan(bound).any():
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(e == 0.0, 0.0, e / bound)
    return float(np.max(q)) if q.size else 0.0


def check(form, A, L, X, rows_seed=0, full=True):
    """Both criteria on one problem's outputs.  Returns {"L": worst |R| / bound_L, "X": worst |X L - I| / bound_X, and for
    bs >= 512 "L_rows", "X_rows": the same in longdouble on the row set}; a ratio <= 1 passes, NaN outputs give inf.
    full = False stops after the float64 evaluation when that already fails (the mutation checks)."""
    n = form.n
    Lc, Xc = clean(form, L, X)
    if np.isnan(Lc).any() or np.isnan(Xc).any():
        return {"L": float("inf"), "X": float("inf")}
    b = bounds(form, Lc, Xc)
    if b is None:
        return {"L": float("inf"), "X": float("inf")}
    bL, bX, M, XLabs = b
    Al = np.tril(A)
    wide_L, wide_X = g(n + 2) * M, g(n + 2) * XLabs
    if form.xsplit:
        p = form.xsplit
        XLabs_d = np.zeros_like(XLabs)
        for s in (slice(0, p), slice(p, n)):
            XLabs_d[s, s] = np.abs(Xc[s, s]) @ np.abs(Lc[s, s])
        wide_X = g(n + 2) * XLabs_d

    def x_resid(prod):
        """X L - I on the blocks the form inverts (the split form's X[b, a] L[a, a] + X[b, b] L[b, a] is not a residual)."""
        r = prod - np.eye(n, dtype=prod.dtype)
        if form.xsplit:
            r[form.xsplit:, :form.xsplit] = 0
        return r

    out = {}
    if n <= 256 and LONGDOUBLE_OK:
        R = Al.astype(LD) - _ld_lower_products(Lc, Lc)
        out["L"] = _ratio(np.abs(np.tril(R)), bL)
        Xl, Ll = Xc.astype(LD), Lc.astype(LD)
        XL = np.zeros((n, n), LD)
        for r0 in range(0, n, 64):
            XL[r0:r0 + 64, :r0 + 64] = Xl[r0:r0 + 64, :r0 + 64] @ Ll[:r0 + 64, :r0 + 64]
        out["X"] = _ratio(np.abs(np.tril(x_resid(XL))), bX)
        return out
    R = Al - np.tril(Lc @ Lc.T)
    out["L"] = _ratio(np.abs(R), bL + wide_L)
    out["X"] = _ratio(np.abs(np.tril(x_resid(Xc @ Lc))), bX + wide_X)
    if n <= 256 or (not full and max(out.values()) > 1.0):
        return out
    rows = row_set(n, rows_seed)
    extra_L = 0.0 if LONGDOUBLE_OK else wide_L[rows]
    extra_X = 0.0 if LONGDOUBLE_OK else wide_X[rows]
    Rr = Al[rows].astype(LD) - _ld_lower_products(Lc, Lc, rows)
    mask = np.arange(n)[None, :] <= rows[:, None]
    out["L_rows"] = _ratio(np.where(mask, np.abs(Rr), 0), bL[rows] + extra_L)
    Xl = Xc.astype(LD)
    Ll = Lc.astype(LD)
    XLr = np.zeros((len(rows), n), LD)
    for i, r in enumerate(rows):
        XLr[i, :r + 1] = Xl[r, :r + 1] @ Ll[:r + 1, :r + 1]
    XLr[np.arange(len(rows)), rows] -= 1
    if form.xsplit:
        XLr[rows >= form.xsplit, :form.xsplit] = 0
    out["X_rows"] = _ratio(np.where(mask, np.abs(XLr), 0), bX[rows] + extra_X)
    return out


def structure_errors(form, L0, X0, L, X):
    """What the output contract forbids, as a list of strings (empty: fine).  L0, X0: the buffers as they went in."""
    n, p = form.n, form.xsplit
    up, du = tile_masks(n)
    low = ~up & ~du
    errs = []
    for nm, a0, a in (("L", L0, L), ("X", X0, X)):
        if not np.array_equal(a[up].view(np.uint64), a0[up].view(np.uint64)):
            errs.append(f"{nm}: a tile above the block diagonal was written")
        if not np.all(a[du] == 0.0):
            errs.append(f"{nm}: the strict upper triangle of a diagonal tile is not zero")
        if not np.all(np.diag(a) > 0.0):
            errs.append(f"{nm}: a diagonal entry is not positive")
        m = low.copy()
        if nm == "L" and form.in_slot:
            m[p:, :p] = False
        if np.isnan(a[m]).any():
            errs.append(f"{nm}: NaN in the lower triangle")
    if p and not form.in_slot and not np.array_equal(X[p:, :p].view(np.uint64), L[p:, :p].view(np.uint64)):
        errs.append("X[b, a] is not L[b, a] bit for bit")
    if form.in_slot and not np.all(np.isnan(L[p:, :p])):
        errs.append("in_slot: L[256:, 0:256] was written")
    return errs


# ------------------------------------------------------------------------------------------------ restatements (CPU only)
def tile_factor(T):
    """One 64 x 64 tile: L = chol(T) from its lower triangle, X = L^-1 by forward substitution on the rows of L X = I."""
    Lt = np.linalg.cholesky(np.tril(T) + np.tril(T, -1).T)
    X = np.zeros((64, 64))
    for k in range(64):
        e = np.zeros(64)
        e[k] = 1.0
        X[k] = (e - Lt[k, :k] @ X[:k]) / Lt[k, k]
    return Lt, X


def _x_rows(L, X, lo, hi, b=64):
    """X[r, c] = -X_rr sum_p L[r, p] X[p, c] for the blocks of b inside [lo, hi) (the diagonal blocks of X are there)."""
    for r0 in range(lo + b, hi, b):
        r1 = r0 + b
        X[r0:r1, lo:r0] = -X[r0:r1, r0:r1] @ (L[r0:r1, lo:r0] @ X[lo:r0, lo:r0])


def _x_doubling(L, X, lo, split=0):
    """X21 = -X22 (L21 X11) per level hh = lo, 2 lo, ...; split: the first block column below row `split` is not assembled."""
    n, hh = L.shape[0], lo
    while hh < n:
        for t in range(0, n, 2 * hh):
            c0 = t
            if split and hh >= split and t == 0:
                if hh == split:
                    continue
                c0 = split
            a, b, c = t, t + hh, t + 2 * hh
            X[b:c, c0:b] = -X[b:c, b:c] @ (L[b:c, c0:b] @ X[c0:b, c0:b])
        hh *= 2


def restate(form, A, drop=None, panel_tiles=4):
    """(L, X) of the route's arithmetic in float64 at tile granularity.  drop = (r, c, j, k0): the trailing update of tile
    (r, c) by the columns of tile column j loses the four columns k0 .. k0 + 3 of that tile column (one MFMA k-step)."""
    n, nt = form.n, form.nt
    S = np.tril(A).copy()
    L, X = np.zeros((n, n)), np.zeros((n, n))
    T = lambda r, c: (slice(64 * r, 64 * r + 64), slice(64 * c, 64 * c + 64))

    def update(rows, cols, ks):
        """S[rows, cols] -= L[rows, ks] L[cols, ks]^T on the lower tiles, one subtraction."""
        for r in rows:
            for c in cols:
                if c > r:
                    continue
                P = L[T(r, 0)[0], ks] @ L[T(c, 0)[0], ks].T
                if drop and (r, c) == drop[:2] and ks.start <= 64 * drop[2] + drop[3] < ks.stop:
                    k = 64 * drop[2] + drop[3]
                    P = P - L[T(r, 0)[0], k:k + 4] @ L[T(c, 0)[0], k:k + 4].T
                S[T(r, c)] -= P

    def steps(j0, j1, rend, cend):
        """64-column steps j0 .. j1 - 1: tile, the rows below up to tile row rend, the update of the columns < cend."""
        for j in range(j0, j1):
            L[T(j, j)], X[T(j, j)] = tile_factor(S[T(j, j)])
            for r in range(j + 1, rend):
                L[T(r, j)] = S[T(r, j)] @ X[T(j, j)].T
            update(range(j + 1, rend), range(j + 1, cend), slice(64 * j, 64 * j + 64))

    if form.route in (ROUTE_FUSED,) or (form.route == ROUTE_STEPS and form.kmax == 64 * nt):
        steps(0, nt, nt, nt)
    elif form.route in (ROUTE_BIG_ONE, ROUTE_STEPS):
        pw = form.kmax // 64
        for j0 in range(0, nt, pw):
            steps(j0, j0 + pw, nt, j0 + pw)
            update(range(j0 + pw, nt), range(j0 + pw, nt), slice(64 * j0, 64 * (j0 + pw)))
    else:
        for j0 in range(0, nt, 4):
            a = 64 * j0
            if form.inv == "panel_persist":
                steps(j0, j0 + 4, j0 + 4, j0 + 4)
                _x_rows(L[a:a + 256, a:a + 256], X[a:a + 256, a:a + 256], 0, 256)
            else:
                for h0 in (j0, j0 + 2):
                    steps(h0, h0 + 2, h0 + 2, h0 + 2)
                    o = 64 * h0
                    X[o + 64:o + 128, o:o + 64] = -X[o + 64:o + 128, o + 64:o + 128] @ (L[o + 64:o + 128, o:o + 64] @ X[o:o + 64, o:o + 64])
                    if h0 == j0:
                        L[a + 128:a + 256, a:a + 128] = S[a + 128:a + 256, a:a + 128] @ X[a:a + 128, a:a + 128].T
                        update(range(j0 + 2, j0 + 4), range(j0 + 2, j0 + 4), slice(a, a + 128))
                X[a + 128:a + 256, a:a + 128] = -X[a + 128:a + 256, a + 128:a + 256] @ (L[a + 128:a + 256, a:a + 128] @ X[a:a + 128, a:a + 128])
            if j0 + 4 < nt:
                L[a + 256:, a:a + 256] = S[a + 256:, a:a + 256] @ X[a:a + 256, a:a + 256].T
                update(range(j0 + 4, nt), range(j0 + 4, nt), slice(a, a + 256))
    if form.route == ROUTE_FUSED and form.rows_upto == n:
        _x_rows(L, X, 0, n)
    elif form.route == ROUTE_PANELS256:
        _x_doubling(L, X, 256, form.xsplit)
    else:
        _x_doubling(L, X, 64)
    if form.xsplit:
        p = form.xsplit
        X[p:, :p] = L[p:, :p]
        if form.in_slot:
            L[p:, :p] = np.nan
    return L, X


# ------------------------------------------------------------------------------------------------ cases and the hook
@dataclass(frozen=True)
class Case:
    """One call of gmrf_test_potrf_route.  panel_tiles: what GMRF_PANEL_TILES the process runs under (read once per process)."""
    n: int
    batch: int = 1
    bits: int = 0
    cmin: int = 0
    keep_l: int = 1
    family: str = "dominant"
    seed: int = 1
    panel_tiles: int = 4

    @property
    def form(self):
        return plan(self.n, self.batch, self.bits, self.cmin, self.keep_l, self.panel_tiles)

    @property
    def probs(self):
        return problems(self.family, self.n, self.seed, self.batch)

    def alone(self, p):
        """Problem p as a call of its own on the batch's route (set_eager bit 1 << 1: the batch routes at batch 1)."""
        f, n, s, _ = self.probs[p]
        return Case(self.n, 1, self.bits | BIT_BATCH_ROUTES, self.cmin, self.keep_l, f, s, self.panel_tiles), self.probs[p]


def run_hook(lib, pkg, case, mats=None):
    """One call.  mats: the problems' matrices if not the case's own (the non-SPD tests).  Returns (L0, X0, L, X, info, route)
    with the buffers as [batch][n][n]."""
    import ctypes as C
    if mats is None:
        mats = [matrix(p) for p in case.probs]
    S, L, X = build_buffers(mats)
    L0, X0 = L.copy(), X.copy()
    info = C.c_int32(-1)
    route = (C.c_int32 * 4)(-1, -1, -1, -1)
    st = lib.gmrf_test_potrf_route(0, case.n, case.batch, case.bits, case.cmin, case.keep_l, pkg._cabi.ptr(S), pkg._cabi.ptr(L),
                                   pkg._cabi.ptr(X), C.byref(info), route)
    pkg._cabi.check(st)
    return L0, X0, L, X, info.value, tuple(route)


def verify(case, out, mats=None, skip=()):
    """Route, structure and both criteria of every problem of a call (but those in `skip`).  Returns the worst ratios, prints them
    first.  Raises AssertionError with what failed."""
    form = case.form
    L0, X0, L, X, info, route = out
    assert route[:3] == (form.route, form.persist, form.xsplit), (route, form)
    assert route[3] == 0, "a persistent wait gave up"
    if mats is None:
        mats = [matrix(p) for p in case.probs]
    worst = {}
    for p in range(case.batch):
        if p in skip:
            continue
        errs = structure_errors(form, L0[p], X0[p], L[p], X[p])
        assert not errs, (p, errs)
        r = check(form, mats[p], L[p], X[p], rows_seed=case.seed + p)
        print(f"potrf {case} problem {p} {case.probs[p][0]}: " + " ".join(f"{k}={v:.3g}" for k, v in r.items()))
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
        assert all(v <= 1.0 for v in r.values()), (case, p, r)
    return worst
