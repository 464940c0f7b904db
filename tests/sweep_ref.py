"""The block sweep products out = [b -] Mat x  /  [b -] Mat^T x of csrc/sweep.hpp restated for the tests (no GPU, no library):

* the route -- which of the sixteen kernel instantiations launch_sweep takes, on which grid, and which shapes a kernel cannot
  compute -- written from the kernels' own tilings (NOT from the host code's control flow: the CPU test compares the two);
* the products sweep_launches issues for a handle's layout (coupling product, full triangular product, the three parts of the
  split form) and the one the batched factorisation's forward solve issues;
* the operand generator: what the contract says is not read holds NaN, what the factor leaves as zeros holds zeros, the panel is
  prefilled with a sentinel;
* the reference in np.longdouble over the contract's range with the per-cell bound
      |out - ref| <= (L + 3) 2^-53 (|b| + sum_k |a_k| |x_k|),      L = the number of terms of the cell's sum.
  Derivation: L products accumulated by fused or unfused multiply-adds in ANY order, partial sums combined by further additions
  (lanes, waves, LDS reductions: every term passes at most L roundings on its way to the total, since a sum of L terms has at
  most L - 1 additions of non-zero partial sums above any leaf plus the leaf's own), is within gamma_L sum |a||x| of the exact
  sum (Higham, Accuracy and Stability, 3.1 / 4.2: the bound holds for every summation order); the subtraction from b rounds
  once more, (1 + delta) on both: gamma_(L+1) (|b| + sum |a||x|).  gamma_(L+1) = (L + 1) u / (1 - (L + 1) u) <= (L + 3) u for
  every L < 2^51.  Adding an exact zero (an idle lane, a stored zero right of the diagonal) rounds nothing.  The sibling of
  tests/spmm_ref.py's (L + 2) u, one more for the addend.
"""
import numpy as np

U = np.longdouble(2.0) ** -53
SENTINEL = -1.2345e300

# ---------------------------------------------------------------------------------------------------- the kernels' constants
NAMES = {1: "sweep_mm<false,false>", 2: "sweep_mm<false,true>", 3: "sweep_mm<true,false>", 4: "sweep_mm<true,true>",
         5: "sweep_gemv_n<false>", 6: "sweep_gemv_n<true>", 7: "sweep_gemv_n_short<false>", 8: "sweep_gemv_n_short<true>",
         9: "sweep_gemv_n4<false>", 10: "sweep_gemv_n4<true>", 11: "sweep_gemv_t<false,8>", 12: "sweep_gemv_t<true,8>",
         13: "sweep_gemv_t<false,16>", 14: "sweep_gemv_t<true,16>", 15: "sweep_gemv_t<false,32>", 16: "sweep_gemv_t<true,32>"}
MM, GEMV_N, GEMV_SHORT, GEMV_N4, GEMV_T8, GEMV_T16, GEMV_T32 = 1, 5, 7, 9, 11, 13, 15     # the non-triangular id of each family
MM_TILE = 16              # sweep_mm: a workgroup owns 16 right-hand sides x 16 outputs ...
MM_KGROUP = 8             # ... and its four waves take K in groups of 8 (two MFMAs of 4)
ROWS_PER_WAVE4 = 4        # sweep_gemv_n_short / sweep_gemv_n4: rows per wave, four waves per workgroup
SHORT_PIECES = 2          # sweep_gemv_n_short: 16-byte pieces of a row per lane -> rows of at most 64 * 2 * 2 elements
N4_MAX = 768              # launch_sweep: beyond this one row per wave (sweep_gemv_n) has enough loads in flight
WIDE_WORKGROUPS = 512     # launch_sweep: 32-column blocks when the batch supplies this many workgroups (two per CU)
MAX_GRID_Z = 65535
REFUSED = (0, 0, 0, 0)


def fam(base, tri):
    return base + (1 if tri else 0)


def mm_id(trans, tri):
    return 1 + 2 * int(bool(trans)) + int(bool(tri))


def kernel_route(kid, trans, tri, kp, rows, kdim, nprob, has_kst=False, has_mend=False):
    """(id, gx, gy, gz) of kernel `kid` on this shape, or REFUSED when the kernel itself cannot compute it."""
    if not 1 <= kid <= 16 or rows <= 0 or kdim <= 0 or kp <= 0 or not 0 < nprob <= MAX_GRID_Z:
        return REFUSED
    if tri and rows != kdim:
        return REFUSED
    if (kid % 2 == 0) != bool(tri):
        return REFUSED
    if kid <= 4:
        if (kid >= 3) != bool(trans) or kp == 1 or kp % MM_TILE or kp // MM_TILE > MAX_GRID_Z or rows % MM_TILE or kdim % MM_KGROUP:
            return REFUSED
        return (kid, rows // MM_TILE, kp // MM_TILE, nprob)
    if kp != 1:
        return REFUSED
    if kid <= 10:
        if trans:
            return REFUSED
        if kid <= 6:
            return (kid, (rows + 3) // 4, 1, nprob)                  # one row per wave, four waves
        rows_per_wg = 4 * ROWS_PER_WAVE4
        if rows % rows_per_wg or kdim % 2:
            return REFUSED
        if kid <= 8 and (kdim > 64 * 2 * SHORT_PIECES or has_kst):
            return REFUSED
        return (kid, rows // rows_per_wg, 1, nprob)
    if not trans:
        return REFUSED
    cw = 8 if kid <= 12 else 16 if kid <= 14 else 32
    if rows < cw or rows % cw:
        return REFUSED
    ncb = rows // cw
    return (kid, (ncb + 1) // 2 if tri else ncb, 1, nprob)


def route(trans, tri, kp, rows, kdim, nprob, narrow=0, has_kst=False, has_mend=False):
    """launch_sweep's choice, then the chosen kernel's own preconditions."""
    if kp != 1:
        kid = mm_id(trans, tri)
    elif not trans:
        four_rows = rows % 16 == 0 and kdim % 2 == 0
        if four_rows and kdim <= 64 * 2 * SHORT_PIECES and not has_kst:
            kid = fam(GEMV_SHORT, tri)
        elif four_rows and nprob >= 8 and kdim <= N4_MAX:
            kid = fam(GEMV_N4, tri)
        else:
            kid = fam(GEMV_N, tri)
    else:
        ncb32 = rows // 32
        wide = nprob >= 8 and rows % 32 == 0 and ((ncb32 + 1) // 2 if tri else ncb32) * nprob >= WIDE_WORKGROUPS
        kid = fam(GEMV_T32 if wide else GEMV_T8 if (narrow and rows % 8 == 0) else GEMV_T16, tri)
    return kernel_route(kid, trans, tri, kp, rows, kdim, nprob, has_kst, has_mend)


# ---------------------------------------------------------------------------------------------------- today's products
SWEEP_PERSIST_XMAX = 1024


def planned_xsplit(bsp, cmin, nprob):
    """The split point of the block inverses a handle's factorisation leaves (0: none): batches on the 256-column panel route
    (blocks of 8 tiles and more, a multiple of 4), a coupling window that starts at cmin >= 256; the largest power of two <= cmin."""
    nt = bsp // 64
    if nprob == 1 or nt < 8 or nt % 4:
        return 0
    p = 256
    while 2 * p <= cmin:
        p *= 2
    return p if cmin >= 256 and p < bsp else 0


def via_gemm(bsp, kp, nprob):
    return kp % 64 == 0 and nprob * (bsp // 64) * (kp // 64) >= 128


def _prod(name, trans, tri, kp, rows, kdim, nprob, narrow, has_kst=False, has_mend=False):
    return dict(name=name, trans=trans, tri=tri, kp=kp, rows=rows, kdim=kdim, nprob=nprob, narrow=narrow, has_kst=has_kst, has_mend=has_mend)


def coupling_product(bsp, cmin, rmax, kp, nprob, backward):
    """P_i -= C y_prev (forward: rows < rmax, sums over the window's columns inside the staircase) / P_i -= C^T x_next."""
    narrow = int(nprob < 8 and 512 <= bsp <= SWEEP_PERSIST_XMAX)
    wc = bsp - cmin
    # (both staircase pointers are set on either direction: sweep_launches sets them once)
    return _prod("coupling", backward, False, kp, wc if backward else rmax, rmax if backward else wc, nprob, narrow, True, True)


def block_products(bsp, xsplit, kp, nprob, backward):
    """y_i = Linv_i t: the full triangular product, or the three parts of the split form [X_aa 0; L_ba X_bb] in their order."""
    narrow = int(nprob < 8 and 512 <= bsp <= SWEEP_PERSIST_XMAX)
    if xsplit <= 0:
        return [_prod("full", backward, True, kp, bsp, bsp, nprob, narrow)]
    p, q = xsplit, bsp - xsplit
    parts = [_prod("aa", backward, True, kp, p, p, nprob, narrow),
             _prod("ba", backward, False, kp, p if backward else q, q if backward else p, nprob, narrow),
             _prod("bb", backward, True, kp, q, q, nprob, narrow)]
    return parts[::-1] if backward else parts


def products(bsp, cmin, rmax, xsplit, kp, nprob, backward):
    """The launch_sweep calls of one block step of sweep_launches (none when the step goes through the GEMM)."""
    if via_gemm(bsp, kp, nprob):
        return []
    return [coupling_product(bsp, cmin, rmax, kp, nprob, backward)] + block_products(bsp, xsplit, kp, nprob, backward)


def factor_forward_product(nprob):
    """The batched factorisation's forward solve on its last 256-column panel: y_P = X_P t_P."""
    return _prod("factor forward", False, True, 1, 256, 256, nprob, 0)


def route_of(pr):
    return route(pr["trans"], pr["tri"], pr["kp"], pr["rows"], pr["kdim"], pr["nprob"], pr["narrow"], pr["has_kst"], pr["has_mend"])


# ---------------------------------------------------------------------------------------------------- operands
def _even_beyond(n, by=2):
    n += by
    return n + (n & 1)


class Case:
    """One product with its operands.  sub: "none" (out = Mat x), "apart" (out = b - Mat x, b elsewhere), "inplace" (b is out).
    kst / mend: lists of one entry per 64 rows (or None).  Leading dimensions are even and beyond the extent, the per-problem
    strides differ from one another and leave gaps; the panel holds the inputs of all problems, then the outputs, then the addends."""

    def __init__(self, trans, tri, kp, rows, kdim, nprob=1, narrow=0, kst=None, mend=None, sub="none", seed=0, p0=0):
        self.trans, self.tri, self.kp, self.rows, self.kdim, self.nprob, self.narrow = bool(trans), bool(tri), kp, rows, kdim, nprob, narrow
        self.kst = None if kst is None else np.asarray(kst, np.int32)
        self.mend = None if mend is None else np.asarray(mend, np.int32)
        self.sub, self.seed, self.p0 = sub, seed, p0
        srows, scols = (kdim, rows) if trans else (rows, kdim)          # the stored block: [k][m] transposed, [m][k] otherwise
        self.srows, self.scols = srows, scols
        self.ld = _even_beyond(scols)
        self.pMat = srows * self.ld + 6
        self.nMat = nprob * self.pMat
        self.ldx, self.ldo = _even_beyond(kdim), _even_beyond(rows, 4)
        self.ldb = self.ldo if sub == "inplace" else _even_beyond(rows, 6)
        self.pXin, self.pOut = kp * self.ldx + 2, kp * self.ldo + 3
        self.pBin = self.pOut if sub == "inplace" else kp * self.ldb + 5
        self.x_off = 2
        self.o_off = self.x_off + nprob * self.pXin + 1
        self.b_off = -1 if sub == "none" else self.o_off if sub == "inplace" else self.o_off + nprob * self.pOut + 1
        self.nP = (self.b_off + nprob * self.pBin if sub == "apart" else self.o_off + nprob * self.pOut) + 3
        self._ref = self._blocks = None

    # -- description
    def desc(self):
        return np.array([self.trans, self.tri, self.kp, self.rows, self.kdim, self.nprob, self.narrow, self.kst is not None,
                         self.mend is not None, self.ld, self.ldx, self.ldb if self.sub != "none" else 0, self.ldo, self.pMat, self.pXin,
                         self.pBin if self.sub != "none" else 0, self.pOut], np.int64)

    def route(self):
        return route(self.trans, self.tri, self.kp, self.rows, self.kdim, self.nprob, self.narrow, self.kst is not None, self.mend is not None)

    def forced(self, kid):
        return kernel_route(kid, self.trans, self.tri, self.kp, self.rows, self.kdim, self.nprob, self.kst is not None, self.mend is not None)

    # -- the contract's range as a mask [m][k] over (output, term)
    def mask(self):
        m, k = np.arange(self.rows)[:, None], np.arange(self.kdim)[None, :]
        live = np.ones((self.rows, self.kdim), bool)
        if self.tri:
            live &= (k >= m) if self.trans else (k <= m)
        if self.kst is not None:
            live &= k >= self.kst[m // 64]
        if self.mend is not None:
            live &= k < self.mend[m // 64]
        return live

    # -- values: problem p0 + p of a case does not depend on the batch it comes in
    def _rng(self, p, what):
        return np.random.default_rng([4242 + self.seed, self.p0 + p, what])

    def blocks(self):
        """(nprob, srows, ld) views' values: standard normal where the contract reads, NaN where it does not, exact zeros in the
        strict upper triangles of the diagonal 64 x 64 tiles of a triangular block."""
        if self._blocks is not None:
            return self._blocks
        out = np.full((self.nprob, self.srows, self.ld), np.nan)
        live = self.mask().T if self.trans else self.mask()            # as stored
        i, j = np.arange(self.srows)[:, None], np.arange(self.scols)[None, :]
        zero = (j > i) & (i // 64 == j // 64) if self.tri else np.zeros_like(live)
        for p in range(self.nprob):
            v = self._rng(p, 0).standard_normal((self.srows, self.scols))
            out[p, :, :self.scols] = np.where(live, v, np.where(zero, 0.0, np.nan))
        self._blocks = out
        return out

    def mat_buffer(self):
        buf = np.full(self.nMat, np.nan)
        B = self.blocks()
        for p in range(self.nprob):
            buf[p * self.pMat: p * self.pMat + self.srows * self.ld] = B[p].ravel()
        return buf

    def x_values(self):
        return np.stack([self._rng(p, 1).standard_normal((self.kp, self.kdim)) for p in range(self.nprob)])

    def b_values(self):
        return np.stack([self._rng(p, 2).standard_normal((self.kp, self.rows)) for p in range(self.nprob)])

    def _cells(self, off, ldr, pstride, n):
        p, r, c = np.arange(self.nprob)[:, None, None], np.arange(self.kp)[None, :, None], np.arange(n)[None, None, :]
        return off + p * pstride + r * ldr + c

    def out_cells(self):
        return self._cells(self.o_off, self.ldo, self.pOut, self.rows)

    def panel(self):
        """The panel before the call: sentinel everywhere, NaN in the pads behind each input vector, inputs and addends live."""
        P = np.full(self.nP, SENTINEL)
        pad = self._cells(self.x_off, self.ldx, self.pXin, self.ldx)[:, :, self.kdim:]
        P[pad.ravel()] = np.nan
        P[self._cells(self.x_off, self.ldx, self.pXin, self.kdim).ravel()] = self.x_values().ravel()
        if self.sub != "none":
            P[self._cells(self.b_off, self.ldb, self.pBin, self.rows).ravel()] = self.b_values().ravel()
        return P

    # -- reference
    def weights(self, p, blocks=None):
        """Problem p's block as [m][k] over (output, term), zero outside the contract's range."""
        B = (self.blocks() if blocks is None else blocks)[p, :, :self.scols]
        return np.where(self.mask(), B.T if self.trans else B, 0.0)

    def reference(self):
        """(ref, bound), both (nprob, kp, rows) longdouble."""
        if self._ref is None:
            live, B, X = self.mask(), self.blocks(), self.x_values()
            L = live.sum(axis=1).astype(np.longdouble)[None, :]
            ref = np.zeros((self.nprob, self.kp, self.rows), np.longdouble)
            mag = np.zeros_like(ref)
            for p in range(self.nprob):
                W = self.weights(p, B).astype(np.longdouble)
                Xp = X[p].astype(np.longdouble)
                for r in range(self.kp):
                    ref[p, r] = (W * Xp[r][None, :]).sum(axis=1)
                    mag[p, r] = (np.abs(W) * np.abs(Xp[r])[None, :]).sum(axis=1)
            if self.sub != "none":
                b = self.b_values().astype(np.longdouble)
                ref, mag = b - ref, mag + np.abs(b)
            self._ref = (ref, (L + 3) * U * mag)
        return self._ref

    def check(self, out, what=""):
        """Every output cell finite and within its bound; returns the worst error / bound ratio."""
        ref, bound = self.reference()
        out = np.asarray(out, np.float64).reshape(ref.shape)
        assert np.all(np.isfinite(out)), f"{what}: non-finite outputs at (problem, rhs, row) {np.argwhere(~np.isfinite(out))[:4].tolist()}"
        err = np.abs(out.astype(np.longdouble) - ref)
        bad = np.argwhere(err > bound)
        assert len(bad) == 0, (f"{what}: {len(bad)} cells beyond the bound, first (problem, rhs, row) {bad[:4].tolist()}, "
                               f"err {err[tuple(bad[0])]}, bound {bound[tuple(bad[0])]}")
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(bound > 0, err / bound, 0)
        return float(ratio.max())

    def check_panel(self, before, after, what=""):
        """The whole panel after the call: the outputs within their bounds, every other cell -- sentinels, NaN pads, inputs, the
        addends that are not outputs -- bit for bit what it was.  Returns (outputs (nprob, kp, rows), worst ratio)."""
        cells = self.out_cells()
        rest = np.ones(self.nP, bool)
        rest[cells.ravel()] = False
        same = before.view(np.uint64)[rest] == after.view(np.uint64)[rest]
        assert np.all(same), f"{what}: {np.count_nonzero(~same)} cells outside the outputs changed, first {np.flatnonzero(rest)[~same][:4].tolist()}"
        out = after[cells]
        return out, self.check(out, what)


# ---------------------------------------------------------------------------------------------------- fp64 emulations
def emulate(case, order="ascending", mutate=None):
    """The product in float64 on the host, problem 0 ... nprob - 1: `order` ascending (one chain per cell) or pairwise (a tree).
    mutate: None, or one of the defects the reference must catch --
      "last term"   every cell's last term dropped          "k group"    one 8-wide group of terms dropped from every cell that has it
      "tri short"   one triangular row one element short     "stair 64"   the staircase bound of the second tile moved by 64
      "float32"     accumulation in float32                  "added"      the addend added instead of subtracted."""
    live = case.mask()
    if mutate == "last term":
        last = case.kdim - 1 - np.argmax(live[:, ::-1], axis=1)
        live = live.copy()
        live[np.arange(case.rows), last] = False
    elif mutate == "k group":
        live = live.copy()
        g = 8 * ((case.kdim // 2) // 8)
        live[:, g:g + 8] = False
    elif mutate == "tri short":
        assert case.tri
        live = live.copy()
        m = case.rows // 2
        live[m, m] = False
    elif mutate == "stair 64":
        live = live.copy()
        if case.kst is not None:
            live[64:128, case.kst[1]:case.kst[1] + 64] = False
        else:
            live[64:128, case.mend[1] - 64:case.mend[1]] = False
    acc_t = np.float32 if mutate == "float32" else np.float64
    B, X = case.blocks(), case.x_values()
    out = np.zeros((case.nprob, case.kp, case.rows))
    for p in range(case.nprob):
        W = np.where(live, (B[p, :, :case.scols].T if case.trans else B[p, :, :case.scols]), 0.0)
        for r in range(case.kp):
            if order == "ascending":
                acc = np.zeros(case.rows, acc_t)
                for k in range(case.kdim):
                    acc = (acc + (W[:, k] * X[p, r, k]).astype(acc_t)).astype(acc_t)
            else:
                t = (W * X[p, r][None, :]).astype(acc_t)
                while t.shape[1] > 1:
                    if t.shape[1] % 2:
                        t = np.concatenate([t, np.zeros((case.rows, 1), acc_t)], axis=1)
                    t = (t[:, 0::2] + t[:, 1::2]).astype(acc_t)
                acc = t[:, 0]
            out[p, r] = acc.astype(np.float64)
    if case.sub != "none":
        b = case.b_values()
        out = b + out if mutate == "added" else b - out
    return out
