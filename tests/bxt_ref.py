"""The coupling step of a factorisation, C_i = B_i Linv_{i-1}^T and the clearing of the Schur block before S = D_i - C_i C_i^T
(csrc/gmrf_hip.hip: build_symbolic, coupling_route, launch_coupling; csrc/misc_kernels.hpp: spmm_bxt, spmm_bxt_tiles), restated
in NumPy: the patterns of the test cases, the host plan (window, staircase, row pointers, tile groups, LDS gate), the route rule,
the longdouble reference with its derived bound and the rules for what a launch may leave unwritten, unread and untouched.

Bound.  Every route forms C[r][c] as one fma chain over the L_r entries of row r of B_i; padding entries and the structural
zeros of the dense image add exact zeros in whatever order.  The forward error of a sum of L products in any order is at most
gamma_L = L u / (1 - L u) times sum |b||x| (u = 2^-53), so |C - ref| <= (L_r + 1) u sum_j |B[r][j]| |X[c][j]|: the + 1 covers
1 / (1 - L u) for L <= 512 and the reference's own rounding at 2^-64.  Where that sum is 0 the cell is +-0 exactly."""
import numpy as np

U = 2.0 ** -53
SENT = np.uint64(0x7FF80000C0DEC0DE)             # a NaN no kernel computes: what nobody wrote still holds it, bit for bit
NCH_LIST = (1, 2, 3, 4, 6, 8, 12, 16, 24, 48)
DENSE, BXT, TILES = 0, 1, 2
FILL_NONE, FILL_ZERO_ROWS, FILL_ZERO_ROLE, FILL_SCATTER_ROLE = 0, 1, 2, 3
SW_DENSE_COUPLING, SW_NO_SCATTER_FOLD = 1 << 3, 1 << 17
ROUTE_NAMES = {DENSE: "dense", BXT: "spmm_bxt", TILES: "spmm_bxt_tiles"}


def next_pow2(x):
    p = 1
    while p < x:
        p *= 2
    return p


def sentinel(n):
    return np.full(n, SENT, np.uint64).view(np.float64)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ------------------------------------------------------------------------------------------------ patterns
class Pattern:
    """Block-tridiagonal Q of N blocks of size bs from explicit entry sets: lower[i] (i >= 1) = (row, column) pairs of B_i in
    block coordinates; D_i = the diagonal, dominant, and a few off-diagonal entries in BOTH triangles (the library keeps the
    lower one: split_csc).  CSC arrays 0-based; values(p): problem p's nzval in CSC order (another seed each, not a scale)."""

    def __init__(self, bs, lower, N=3, name=""):
        self.bs, self.N, self.name = bs, N, name
        self.n = bs * N
        self.bsp = 64 * next_pow2((bs + 63) // 64)
        assert len(lower) == N and lower[0] is None
        self.lower = [None]
        for i in range(1, N):
            e = sorted(set((int(r), int(c)) for r, c in lower[i]))
            assert all(0 <= r < bs and 0 <= c < bs for r, c in e)
            self.lower.append(np.array(e, np.int64).reshape(-1, 2))
        self.diag = []
        for i in range(N):
            e = {(r, r) for r in range(bs)}
            for k in range(0, bs - 3, 7):                 # a few off-diagonal entries, both triangles
                e.add((k + 3, k))
                e.add((k, k + 2))
            if bs > 70:
                e.add((bs - 1, 1 + i))                    # a long-range one, another cell in every block
                e.add((i, bs - 2))
            self.diag.append(np.array(sorted(e), np.int64))
        rows, cols = [], []
        for i in range(N):
            rows.append(self.diag[i][:, 0] + i * bs)
            cols.append(self.diag[i][:, 1] + i * bs)
            if i > 0:
                rows.append(self.lower[i][:, 0] + i * bs)
                cols.append(self.lower[i][:, 1] + (i - 1) * bs)
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        order = np.lexsort((rows, cols))
        self.rowval = np.ascontiguousarray(rows[order])
        self.colidx = np.ascontiguousarray(cols[order])
        self.colptr = np.zeros(self.n + 1, np.int64)
        np.add.at(self.colptr, self.colidx + 1, 1)
        self.colptr = np.cumsum(self.colptr)
        self.nnz = len(self.rowval)
        self._pos = {(int(r), int(c)): k for k, (r, c) in enumerate(zip(self.rowval, self.colidx))}

    def values(self, p):
        rng = np.random.default_rng(1000 + 17 * p)
        v = rng.uniform(-1.0, 1.0, self.nnz)
        v[np.abs(v) < 0.05] = 0.5
        dg = self.rowval == self.colidx
        v[dg] = 8.0 + rng.uniform(0.0, 1.0, int(dg.sum()))
        return v

    def lower_vals(self, i, vals):
        """B_i's values in (row, column) order."""
        e = self.lower[i]
        return np.array([vals[self._pos[(int(r) + i * self.bs, int(c) + (i - 1) * self.bs)]] for r, c in e], np.float64)

    def diag_lower(self, i, vals):
        """D_i's kept entries (row >= column) and their values."""
        e = self.diag[i][self.diag[i][:, 0] >= self.diag[i][:, 1]]
        return e, np.array([vals[self._pos[(int(r) + i * self.bs, int(c) + i * self.bs)]] for r, c in e], np.float64)


# ------------------------------------------------------------------------------------------------ plan
def plan(pat, group_tiles):
    """build_symbolic's coupling part and set_layout's kst, restated."""
    N, bsp = pat.N, pat.bsp
    P = {}
    cmin, rmax = bsp, 0
    first = np.full(bsp // 64, bsp, np.int64)
    for i in range(1, N):
        for r, c in pat.lower[i]:
            cmin = min(cmin, c)
            rmax = max(rmax, r + 1)
            first[r // 64] = min(first[r // 64], c)
    if rmax == 0:
        cmin, rmax, first[0] = 0, 64, 0
    cmin = cmin // 64 * 64
    rmax = min(bsp, (rmax + 63) // 64 * 64)
    first = first[:rmax // 64]
    nrt, ntile = rmax // 64, bsp // 64
    kst = np.zeros(ntile, np.int32)
    run = bsp - 64
    for t in range(nrt - 1, -1, -1):
        v = min(max(int(first[t]), cmin), bsp - 64)
        run = min(run, v // 64 * 64)
        kst[t] = run - cmin
    if nrt > 0:
        kst[0] = 0
    kst[nrt:] = bsp - cmin
    # entries in storage order: per block D_i's kept entries, then B_i's rows
    low_first, pos = [0] * N, 0
    for i in range(N):
        pos += int((pat.diag[i][:, 0] >= pat.diag[i][:, 1]).sum())
        low_first[i] = pos
        if i > 0:
            pos += len(pat.lower[i])
    n_entries = pos
    rowptr = np.zeros((N, bsp + 1), np.int32)
    max_row = 0
    for i in range(1, N):
        cnt = np.zeros(bsp + 1, np.int64)
        np.add.at(cnt, pat.lower[i][:, 0] + 1, 1)
        max_row = max(max_row, int(cnt.max()))
        cnt[0] = low_first[i]
        rowptr[i] = np.cumsum(cnt)
    sparse_b = max_row <= 32 and bsp >= 64
    P.update(cmin=cmin, rmax=rmax, first=first, kst=kst, rowptr=rowptr, max_row=max_row, sparse_b=sparse_b, n_entries=n_entries,
             low_first=low_first, bxt_ok=False, ecap=0, nrt=0)
    if not (sparse_b and N > 1):
        return P
    uptr = np.zeros((N, nrt + 1), np.int32)
    gtiles = np.full((N, nrt, 3), -1, np.int32)
    ng = np.zeros(N, np.int32)
    lidx = np.zeros(max(n_entries, 1), np.uint16)
    ucols, ok, pmax = [], True, 0
    for i in range(1, N):
        e = pat.lower[i]
        rp = rowptr[i]
        cols = [sorted(set(int(c) for c in e[(e[:, 0] // 64) == rt][:, 1])) for rt in range(nrt)]
        if any(len(c) > 256 for c in cols):
            ok = False
            break
        taken, g = [False] * nrt, 0
        for rt in range(nrt):
            if taken[rt]:
                continue
            gt = [rt]
            taken[rt] = True
            uni = set(cols[rt])
            for u in range(rt + 1, nrt):
                if len(gt) >= 3 or not group_tiles:
                    break
                if taken[u] or not cols[u]:
                    continue
                tmp = uni | set(cols[u])
                common = len(uni) + len(cols[u]) - len(tmp)
                if 2 * common >= len(cols[u]) and len(tmp) <= 256:
                    gt.append(u)
                    taken[u] = True
                    uni = tmp
            uni = sorted(uni)
            where = {c: k for k, c in enumerate(uni)}
            padded = 0
            for t in gt:
                for q in range(rp[t * 64], rp[t * 64 + 64]):
                    lidx[q] = where[int(e[q - low_first[i], 1])]
                for r in range(t * 64, t * 64 + 64):
                    padded += (int(rp[r + 1] - rp[r]) + 3) // 4 * 4
            pmax = max(pmax, padded)
            gtiles[i, g, :len(gt)] = gt
            uptr[i, g] = len(ucols)
            ucols.extend(uni)
            g += 1
        uptr[i, g:] = len(ucols)
        ng[i] = g
    ecap = max(64, (pmax + 63) // 64 * 64)
    if ok and 38440 + 10 * ecap <= 54272:                                  # spmm_bxt_tiles' LDS: 53 KB
        P.update(bxt_ok=True, ecap=ecap, nrt=nrt, ng=ng, gtiles=gtiles, uptr=uptr, ucols=np.array(ucols, np.int32), lidx=lidx)
    P["pmax"] = pmax
    return P


def zero_wgs(bsp, rm):
    return min(32, max(1, (bsp - rm) * bsp // 16384))


def route_of(pat, P, kind, B, cus, i, switches=0):
    """coupling_route_of: (kind, KM, cw, nch, ncg, ng, grid, fill, zwgs, skip_dead)."""
    bsp, cm, rm = pat.bsp, P["cmin"], P["rmax"]
    W, rch = bsp - cm, (rm + 255) // 256
    km = cw = nch = ncg = ng = grid = zwgs = 0
    fill = FILL_NONE
    if kind == TILES:
        ng = int(P["ng"][i])
        chunks, slots = W // 16, 3 * max(cus, 1)
        best, best_cost = 1, None
        for c in NCH_LIST:
            if c > chunks:
                break
            wgs = -(-chunks // c) * ng * B
            cost = -(-wgs // slots) * (c + 2)
            if best_cost is None or cost < best_cost:
                best, best_cost = c, cost
        nch = best
        ncg = -(-chunks // nch)
        if B == 1 and bsp == pat.bs and not switches & SW_NO_SCATTER_FOLD:
            fill, zwgs = FILL_SCATTER_ROLE, 64
        elif rm < bsp:
            fill, zwgs = FILL_ZERO_ROLE, zero_wgs(bsp, rm)
        grid = (ncg * ng + zwgs) * B
    else:
        if kind == BXT:
            km = 8 if P["max_row"] <= 8 else (16 if P["max_row"] <= 16 else 32)
            cw = 64 if (W // 64) * rch * B >= 512 else (32 if (W // 32) * rch * B >= 512 else 16)
            grid = (W // cw) * rch * B
        if rm < bsp:
            fill = FILL_ZERO_ROWS
    return (kind, km, cw, nch, ncg, ng, grid, fill, zwgs, 0)


def route(pat, P, B, cus, i, switches=0):
    sparse = P["sparse_b"] and not switches & SW_DENSE_COUPLING
    kind = DENSE if not sparse else (TILES if P["bxt_ok"] and P["nrt"] == P["rmax"] // 64 else BXT)
    return route_of(pat, P, kind, B, cus, i, switches)


def with_overrides(pat, P, r, B, cw=0, nch=0, skip_dead=0, fill=0):
    """The route the product hook reports for overrides it admits."""
    kind, km, cw0, nch0, ncg, ng, grid, fill0, zwgs, sd = r
    bsp, cm, rm = pat.bsp, P["cmin"], P["rmax"]
    W, rch = bsp - cm, (rm + 255) // 256
    cw, nch = cw or cw0, nch or nch0
    sd = skip_dead - 1 if skip_dead else sd
    if fill == 1:
        fill0, zwgs = FILL_NONE, 0
    elif fill == 2:
        fill0, zwgs = FILL_ZERO_ROLE, zero_wgs(bsp, rm)
    elif fill == 3:
        fill0, zwgs = FILL_SCATTER_ROLE, 64
    if kind == BXT:
        grid = (W // cw) * rch * B
    elif kind == TILES:
        ncg = -(-(W // 16) // nch)
        grid = (ncg * ng + zwgs) * B
    return (kind, km, cw, nch, ncg, ng, grid, fill0, zwgs, sd)


# ------------------------------------------------------------------------------------------------ operands
def make_x(pat, p, seed=0):
    """Linv_{i-1} of problem p: random lower triangular, zeros above the diagonal (what the factor leaves)."""
    rng = np.random.default_rng(5000 + 31 * p + seed)
    X = np.tril(rng.uniform(-1.0, 1.0, (pat.bsp, pat.bsp)))
    X[np.diag_indices(pat.bsp)] = rng.uniform(0.5, 1.5, pat.bsp)
    return X


def poison_x(pat, P, i, X, kind):
    """NaN where the route may not read: rows < cm; the sparse routes: every column no entry of B_i references; the tile kernel,
    which documents that it fetches nothing right of the diagonal: there too.  The dense GEMM multiplies the structural zeros of
    B's image with columns >= cm (its K range), so only the columns left of cm are poisoned for it."""
    Xd = X.copy()
    cm = P["cmin"]
    Xd[:cm, :] = np.nan
    if kind == DENSE:
        Xd[:, :cm] = np.nan
    else:
        ref = np.zeros(pat.bsp, bool)
        ref[pat.lower[i][:, 1]] = True
        Xd[:, ~ref] = np.nan
        if kind == TILES:
            Xd[np.triu_indices(pat.bsp, 1)] = np.nan
    return Xd


def reference(pat, P, i, bvals, X):
    """(ref, bound) as float64 / longdouble arrays [rm][W] from the CLEAN X (zeros above the diagonal)."""
    cm, rm, bsp = P["cmin"], P["rmax"], pat.bsp
    W = bsp - cm
    Xl = X[cm:, :].astype(np.longdouble)
    Xa = np.abs(Xl)
    ref = np.zeros((rm, W), np.longdouble)
    mag = np.zeros((rm, W), np.longdouble)
    L = np.zeros(rm, np.int64)
    for (r, j), v in zip(pat.lower[i], bvals):
        lv = np.longdouble(v)
        ref[r] += lv * Xl[:, j]
        mag[r] += abs(lv) * Xa[:, j]
        L[r] += 1
    bound = (L[:, None] + 1).astype(np.longdouble) * np.longdouble(U) * mag
    return ref, bound


def emulate(pat, P, i, bvals, X, entries=None):
    """A float64 product over the given entry list (default: B_i's own): what a correct kernel may return."""
    cm, rm = P["cmin"], P["rmax"]
    e = pat.lower[i] if entries is None else entries
    out = np.zeros((rm, pat.bsp - cm))
    for (r, j), v in zip(e, bvals):
        out[r] += v * X[cm:, j]
    return out


def c_image_shape(pat, P, B):
    return (B, max(pat.N - 1, 1), P["rmax"], pat.bsp - P["cmin"])


# ------------------------------------------------------------------------------------------------ checks
def check_c(pat, P, i, B, C_after, refs, what=""):
    """C_after: the whole image [B][N - 1][rm][W] after one launch on an image of sentinels; refs[p] = (ref, bound).  Returns
    (written, worst error / bound, cells compared): written[p] = mask of the window's cells that hold a value."""
    cm, rm, bsp = P["cmin"], P["rmax"], pat.bsp
    img = C_after.reshape(c_image_shape(pat, P, B))
    ib = bits(img)
    outside = np.ones(img.shape[:2], bool)
    outside[:, i - 1] = False
    bad = (ib != SENT) & outside[:, :, None, None]
    assert not bad.any(), (what, "wrote outside block", i, "at (problem, block - 1, row, column)", tuple(np.argwhere(bad)[0]))
    left = np.arange(bsp - cm)[None, :] < P["kst"][np.arange(rm) // 64][:, None]
    worst, cells, written = 0.0, 0, []
    for p in range(B):
        ref, bound = refs[p]
        got = img[p, i - 1]
        isent = ib[p, i - 1] == SENT
        miss = isent & ~left
        assert not miss.any(), (what, "problem", p, "left unwritten right of the staircase at (row, window column)", tuple(np.argwhere(miss)[0]))
        w = ~isent
        err = np.abs(got.astype(np.longdouble) - ref)
        with np.errstate(invalid="ignore"):
            over = w & ~(err <= bound)
        assert not over.any(), (what, "problem", p, "outside the bound at", tuple(np.argwhere(over)[0]),
                                "got", got[tuple(np.argwhere(over)[0])], "ref", float(ref[tuple(np.argwhere(over)[0])]))
        nz = w & (bound > 0)
        if nz.any():
            worst = max(worst, float((err[nz] / bound[nz]).max()))
        cells += int(w.sum())
        written.append(w)
    return written, worst, cells


def check_s(pat, P, i, B, S_after, fill, vals, what=""):
    """The Schur work block [B][bsp][bsp] after one launch on sentinels, exactly."""
    bsp, rm = pat.bsp, P["rmax"]
    S = S_after.reshape(B, bsp, bsp)
    sb = bits(S)
    for p in range(B):
        want = np.full((bsp, bsp), SENT, np.uint64)
        if fill in (FILL_ZERO_ROWS, FILL_ZERO_ROLE):
            want[rm:, :] = 0
        elif fill == FILL_SCATTER_ROLE:
            for r in range(bsp):
                want[r, :64 * (r // 64 + 1)] = 0
            e, v = pat.diag_lower(i, vals[p])
            want[e[:, 0], e[:, 1]] = bits(v)
        bad = sb[p] != want
        assert not bad.any(), (what, "problem", p, "Schur block cell", tuple(np.argwhere(bad)[0]), "holds", S[p][tuple(np.argwhere(bad)[0])])


def tie(a, wa, b, wb, what=""):
    """Two launches agree bit for bit on the cells both wrote (+0 and -0 are the same exact zero)."""
    both = wa & wb
    x, y = a[both], b[both]
    same = (bits(x) == bits(y)) | ((x == 0) & (y == 0))
    assert same.all(), (what, "differ at", tuple(np.argwhere(both)[np.argmin(same)]), x[np.argmin(same)], y[np.argmin(same)])


# ------------------------------------------------------------------------------------------------ cases
def band(bs=128):
    lo1 = [(r, c) for r in range(bs) for c in (r - 1, r, r + 1) if 0 <= c < bs]
    lo2 = [(r, c) for r in range(bs) for c in (r - 2, r, r + 1) if 0 <= c < bs]
    return Pattern(bs, [None, lo1, lo2], name=f"band{bs}")


def window():
    """bs 256: rows < 128, columns >= 64; tile 1 starts at column 192 (in block 2; at 200 in block 1)."""
    lo1 = [(r, 64 + r) for r in range(64)] + [(r, 70 + 2 * r) for r in range(64)] + \
          [(r, 200 + (r - 64) // 2) for r in range(64, 128)] + [(r, 255) for r in range(64, 128, 3)]
    lo2 = [(r, 66 + r) for r in range(64)] + [(r, 64) for r in range(0, 64, 5)] + [(r, 250 - r // 8) for r in range(64)] + \
          [(r, 192 + (r - 64) % 60) for r in range(64, 128)] + [(r, 254) for r in range(64, 128, 2)]
    return Pattern(256, [None, lo1, lo2], name="window")


def ragged(shared=True):
    """bs 320 (bsp 512): columns 192 .. 319, so cm = 192, W = 320, rm = 320.  Tiles 0 - 2 meet the same columns (one group of
    three), tiles 3 and 4 disjoint ones further right (kst = [0, 0, 0, 64, 64]): a 3-tile group beside single tiles."""
    def blk(o):
        e = []
        for r in range(320):
            t, q = r // 64, r % 64
            if t < 3:
                e += [(r, 192 + q), (r, 193 + q), (r, 200 + (q + o) % 64)]
                if r % 7 == o:
                    e += [(r, 300), (r, 319)]
            elif t == 3:
                e += [(r, 256 + (q + o) % 32), (r, 256 + q // 2)]
            else:
                e += [(r, 288 + (q + 2 * o) % 32), (r, 319 - q // 4)]
        return e
    return Pattern(320, [None, blk(0), blk(1)], name="ragged")


ROW_LENGTHS = {8: (0, 1, 3, 4, 5, 8), 16: (0, 1, 3, 4, 5, 8, 9, 16), 32: (0, 1, 3, 4, 5, 8, 9, 16, 17, 32), 33: (0, 1, 3, 4, 5, 8, 9, 16, 17, 32, 33)}


def rows(km):
    """bs 128: row lengths mixed over the rows; block 2 has an empty tile 0.  km 33: one row of 33 entries (the lower blocks go dense)."""
    lens = ROW_LENGTHS[km]

    def blk(o, empty_tile):
        e = []
        for r in range(128):
            if r // 64 == empty_tile:
                continue
            n = lens[(r + o) % len(lens)]
            if km == 33:
                n = 33 if r == 70 else min(n, 32)
            e += [(r, (3 * r + 5 * k + o) % 128) for k in range(n)] if n <= 25 else [(r, (r + 3 * k + o) % 128) for k in range(n)]
        return e
    return Pattern(128, [None, blk(0, -1), blk(1, 0)], name=f"rows{km}")


def ucap(extra=False):
    """bs 512: tile 0 of block 1 meets exactly 256 distinct columns (257 with `extra`)."""
    lo1 = [(r, 4 * r + k) for r in range(64) for k in range(4)] + [(r, r - 3) for r in range(64, 512)] + [(r, r) for r in range(64, 512, 2)]
    if extra:
        lo1.append((10, 256))
    lo2 = [(r, c) for r in range(512) for c in (r - 5, r) if 0 <= c < 512]
    return Pattern(512, [None, lo1, lo2], name="ucap257" if extra else "ucap256")


def lds(over=False):
    """bs 256: tile 0 of block 1 holds 64 rows x 24 entries = 1536 padded entries on columns 0 .. 212 (`over`: one row of 25 ->
    1540); the other tiles meet columns 213 .. 255 only, so tile 0 stays a group of its own, grouped or not."""
    lo1 = [(r, 3 * r + k) for r in range(64) for k in range(24)] + [(r, 213 + r % 43) for r in range(64, 256)]
    if over:
        lo1.append((5, (15 + 24) % 256))
    lo2 = [(r, c) for r in range(256) for c in (r - 1, r) if c >= 0]
    return Pattern(256, [None, lo1, lo2], name="lds1540" if over else "lds1536")


def padded(low_rows_only):
    """bs 100 (bsp 128).  All rows: rm = 128, the pad rows 100 .. 127 are empty.  Rows < 64 only: rm = 64 < bsp."""
    top = 64 if low_rows_only else 100
    lo1 = [(r, c) for r in range(top) for c in (r - 1, r, (r + 37) % 100) if 0 <= c < 100]
    lo2 = [(r, c) for r in range(top) for c in (r, r + 2, (r + 11) % 100) if 0 <= c < 100]
    return Pattern(100, [None, lo1, lo2], name="padded64" if low_rows_only else "padded100")


def greedy_loses():
    """bs 192 (bsp 256): three tiles of 64 x 12 entries on the same columns."""
    lo = [(r, (r % 64 + 5 * k) % 192) for r in range(192) for k in range(12)]
    lo2 = [(r, (r % 64 + 5 * k + 1) % 192) for r in range(192) for k in range(12)]
    return Pattern(192, [None, lo, lo2], name="greedy")


_CASES = {}


def case(name):
    """The shared, unchanged case objects (a pattern is built once)."""
    if name not in _CASES:
        _CASES[name] = {
            "band": lambda: band(128), "window": window, "ragged": ragged,
            "rows8": lambda: rows(8), "rows16": lambda: rows(16), "rows32": lambda: rows(32), "rows33": lambda: rows(33),
            "ucap256": lambda: ucap(False), "ucap257": lambda: ucap(True), "lds1536": lambda: lds(False), "lds1540": lambda: lds(True),
            "padded100": lambda: padded(False), "padded64": lambda: padded(True), "greedy": greedy_loses,
        }[name]()
    return _CASES[name]


ALL_CASES = ("band", "window", "ragged", "rows8", "rows16", "rows32", "rows33", "ucap256", "ucap257", "lds1536", "lds1540",
             "padded100", "padded64", "greedy")

_PLANS, _REFS = {}, {}


def case_plan(name, group_tiles):
    key = (name, bool(group_tiles))
    if key not in _PLANS:
        _PLANS[key] = plan(case(name), group_tiles)
    return _PLANS[key]


def case_refs(name, i, p):
    """(values, B_i's values, clean X, ref, bound) of problem p of a case: computed once, shared, left unchanged."""
    key = (name, i, p)
    if key not in _REFS:
        pat, P = case(name), case_plan(name, True)
        vals = pat.values(p)
        bv = pat.lower_vals(i, vals)
        X = make_x(pat, p, seed=i)
        ref, bound = reference(pat, P, i, bv, X)
        _REFS[key] = (vals, bv, X, ref, bound)
    return _REFS[key]


# ------------------------------------------------------------------------------------------------ the library's side
def lib_plan(cabi, lib, pat, group_tiles, query=None):
    """gmrf_test_coupling_plan as a dict shaped like plan()'s, and the route of `query` = (B, CUs, block, switches) or None."""
    N, bsp = pat.N, pat.bsp
    nrt_max = bsp // 64
    ne = pat.nnz + 1
    scal = np.full(12, -1, np.int64)
    kst = np.full(bsp // 64, -1, np.int32)
    rowptr = np.full((N, bsp + 1), -1, np.int32)
    ng = np.full(N, -1, np.int32)
    gtiles = np.full(N * nrt_max * 3, -7, np.int32)
    uptr = np.full(N * (nrt_max + 1), -1, np.int32)
    ucols = np.full(N * nrt_max * 256 + 1, -1, np.int32)
    lidx = np.full(ne, 0xFFFF, np.uint16)
    cap = np.array([kst.size, rowptr.size, ng.size, gtiles.size, uptr.size, ucols.size, lidx.size], np.int64)
    q = None if query is None else np.array(query, np.int64)
    r = np.full(10, -1, np.int64)
    p = cabi.ptr
    cabi.check(lib.gmrf_test_coupling_plan(pat.n, N, p(pat.colptr), p(pat.rowval), 0, int(bool(group_tiles)), p(scal), p(kst), p(rowptr),
                                           p(ng), p(gtiles), p(uptr), p(ucols), p(lidx), p(cap), p(q), p(r)))
    P = dict(cmin=int(scal[0]), rmax=int(scal[1]), max_row=int(scal[2]), sparse_b=bool(scal[3]), bxt_ok=bool(scal[4]), ecap=int(scal[5]),
             nrt=int(scal[6]), kst=kst, rowptr=rowptr)
    assert scal[7] == kst.size and scal[8] == rowptr.size
    if P["bxt_ok"]:
        nrt = P["nrt"]
        P.update(ng=ng, gtiles=gtiles[:scal[9]].reshape(N, nrt, 3), uptr=uptr[:N * (nrt + 1)].reshape(N, nrt + 1), ucols=ucols[:scal[10]],
                 lidx=lidx[:scal[11]])
    return P, (None if query is None else tuple(int(v) for v in r))
