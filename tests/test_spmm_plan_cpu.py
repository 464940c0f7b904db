"""The sparse products' tile plan and route functions, host only (gmrf_test_spmm_plan needs no device), against their
restatement (tests/spmm_ref.py): every plan number and array on the matrices of the GPU route tests, the route functions at each
of their boundaries, and which of the twelve tiled instantiations (kernel, R, NG) the plan reaches on its own."""
import ctypes as C

import numpy as np
import pytest

from tests import spmm_ref as R

PLAIN, TILES, PAD = R.PLAIN, R.TILES, R.PAD


def host_plan(pkg, lib, A, k=16, ldx=None, ldy=None, x_al=True, y_al=True, xs=0, ys=0, no_pad=False, arrays=False, n_cols=None):
    """gmrf_test_spmm_plan -> dict like spmm_ref.plan plus the routes."""
    ldx, ldy = k if ldx is None else ldx, k if ldy is None else ldy
    geom = np.array([k, ldx, ldy, x_al, y_al, xs, ys, no_pad], np.int64)
    out = np.zeros(12, np.int64)
    n_rows = A.shape[0]
    n_cols = A.shape[1] if n_cols is None else n_cols
    args = (n_rows, n_cols, pkg._cabi.ptr(A.rowptr), pkg._cabi.ptr(A.colidx), 0, pkg._cabi.ptr(geom), pkg._cabi.ptr(out))
    pkg._cabi.check(lib.gmrf_test_spmm_plan(*args, None, None, None, 0, 0))
    keys = ("state", "R", "ucap", "ecap", "ecap_pad", "umax", "tiles", "n_ucols")
    d = dict(zip(keys, (int(v) for v in out[:8])))
    d.update(rows=(int(out[8]), int(out[9])), cols=int(out[10]), tiles_ok=bool(out[11]))
    if arrays and d["state"] == 1:
        up, uc, li = np.full(d["tiles"] + 1, -1, np.int64), np.full(d["n_ucols"], -1, np.int32), np.full(max(A.nnz, 1), 0xffff, np.uint16)
        pkg._cabi.check(lib.gmrf_test_spmm_plan(*args, pkg._cabi.ptr(up), pkg._cabi.ptr(uc), pkg._cabi.ptr(li), len(up), len(uc)))
        d.update(tile_uptr=up, ucols=uc, lidx=li[:A.nnz])
    return d


def from_scipy(Q):
    Q = Q.tocsr()
    Q.sort_indices()
    return R.Csr(Q.shape[0], Q.shape[1], Q.indptr, Q.indices, Q.data)


def gpu_test_matrices():
    m = {f"pad R{r} NG{ng}": R.generate(100, w, p) for (r, ng), (w, p) in R.TABLE.items()}
    m.update({f"lengths R{r} NG{ng}": R.generate(100, w, p, lengths=R.ROW_LENGTHS) for (r, ng), (w, p) in list(R.TABLE.items())[:2]})
    m["unpadded R64 NG7"] = R.generate(100, *R.UNPADDED_64_7)
    m["no plan"] = R.generate(100, *R.NO_PLAN)
    m["entries"] = R.generate(100, 300, 520, replace=True)
    for per in (9, 15, 25, 45):
        m[f"lane group per {per}"] = R.generate(100, 120, per)
    m["tridiagonal"] = R.tridiagonal(1000)
    return m


@pytest.fixture(scope="module")
def matrices(pkg):
    m = gpu_test_matrices()
    for name in ("darcy32", "darcy64"):
        m[name] = from_scipy(pkg.workloads.make(name).Q)
    return m


def test_plan_matches_the_restatement(pkg, lib, matrices):
    for name, A in matrices.items():
        got, ref = host_plan(pkg, lib, A, arrays=True), R.plan(A.shape[0], A.rowptr, A.colidx)
        for key in ("state", "R", "ucap", "ecap", "ecap_pad", "umax", "tiles"):
            assert got[key] == ref[key], (name, key, got[key], ref[key])
        assert got["tiles_ok"] == R.spmv_tiles_ok(A.shape[0], A.rowptr), name
        if ref["state"] != 1:
            continue
        assert np.array_equal(got["tile_uptr"], ref["tile_uptr"]) and np.array_equal(got["ucols"], ref["ucols"]), name
        assert np.array_equal(got["lidx"], ref["lidx"]), name
        # the plan's own invariants, from the library's arrays alone
        Rr, up, uc = got["R"], got["tile_uptr"], got["ucols"]
        tile_of_entry = A.rows() // Rr
        assert np.array_equal(uc[up[tile_of_entry] + got["lidx"]], A.colidx), name
        for t in range(got["tiles"]):
            assert np.all(np.diff(uc[up[t]:up[t + 1]]) > 0), (name, t)


def test_table_matrices_take_the_routes_they_name(pkg, lib):
    """The (width, per) table of the GPU tests, re-confirmed on both sides: each matrix plans the (R, NG) it is named after,
    padded; withheld, the same (R, NG) unpadded."""
    for (r, ng), (w, p) in R.TABLE.items():
        for A in (R.generate(100, w, p), R.generate(100, w, p, lengths=R.ROW_LENGTHS)):
            pl = R.plan(100, A.rowptr, A.colidx)
            if np.diff(A.rowptr).max() == p:                # (fixed row lengths change the plan: only the full table rows are pinned)
                assert (pl["R"], R.rows_route(pl, w, 16, 16, 16)) == (r, (PAD, ng)), (r, ng, pl)
            for no_pad in (False, True):
                got = host_plan(pkg, lib, A, no_pad=no_pad)
                assert (got["R"], got["rows"]) == (pl["R"], R.rows_route(pl, w, 16, 16, 16, no_pad=no_pad))
                assert got["rows"][0] == (TILES if no_pad else PAD)
    A = R.generate(100, *R.UNPADDED_64_7)
    got = host_plan(pkg, lib, A)
    assert (got["R"], got["ecap"], got["ecap_pad"], got["rows"]) == (64, 3840, 0, (TILES, 7))
    assert R.tile_pad_lds_bytes(64, 96, 4032) > 53 * 1024 > 52 * 1024 >= R.tile_lds_bytes(64, 96, 3840)
    A = R.generate(100, *R.NO_PLAN)
    assert host_plan(pkg, lib, A)["state"] == -1 and R.plan(100, A.rowptr, A.colidx)["why"] == {64: "lds", 32: "lds", 16: "lds"}
    A = R.generate(100, 300, 520, replace=True)             # 16 rows x 520 entries > 8192 on at most 300 distinct columns
    assert host_plan(pkg, lib, A)["state"] == -1 and R.plan(100, A.rowptr, A.colidx)["why"] == {64: "entries", 32: "entries", 16: "entries"}


def test_node_major_route_boundaries(pkg, lib):
    A = R.generate(100, *R.TABLE[(64, 10)])
    pl = R.plan(100, A.rowptr, A.colidx)
    n_cols = A.shape[1]
    cases = [dict(k=k) for k in (1, 2, 3, 4, 16, 17, 18)]
    cases += [dict(k=4, ldx=5, ldy=4), dict(k=4, ldx=6, ldy=7), dict(k=4, ldx=6, ldy=10)]
    cases += [dict(x_al=False), dict(y_al=False), dict(xs=30001), dict(ys=30001), dict(xs=30002, ys=30002), dict(no_pad=True)]
    for c in cases:
        k = c.get("k", 16)
        got = host_plan(pkg, lib, A, **c)["rows"]
        assert got == R.rows_route(pl, n_cols, k, c.get("ldx", k), c.get("ldy", k), c.get("x_al", True), c.get("y_al", True),
                                   c.get("xs", 0), c.get("ys", 0), c.get("no_pad", False)), c
        odd = k % 2 or c.get("ldx", k) % 2 or c.get("ldy", k) % 2 or c.get("xs", 0) % 2 or c.get("ys", 0) % 2
        assert (got[0] == PLAIN) == bool(odd or not c.get("x_al", True) or not c.get("y_al", True)), c
    # n_cols * ldx: 32-bit gather offsets in 16-byte units hold up to 2^32 - 2 doubles (the pattern only names small columns)
    ld = 2 ** 16
    assert host_plan(pkg, lib, A, k=16, ldx=ld, n_cols=2 ** 16 - 1)["rows"] == (PAD, 10)
    assert (2 ** 16) * ld == 2 ** 32 and host_plan(pkg, lib, A, k=16, ldx=ld, n_cols=2 ** 16)["rows"] == (PLAIN, 0)
    assert host_plan(pkg, lib, A, k=2, ldx=2, n_cols=2 ** 31 - 1)["rows"] == (PAD, 10)       # n_cols * ldx = 2^32 - 2
    assert host_plan(pkg, lib, A, k=2, ldx=2, n_cols=2 ** 31)["rows"] == (PLAIN, 0)          # 2^32
    assert R.rows_route(pl, 2 ** 31 - 1, 2, 2, 2) == (PAD, 10) and R.rows_route(pl, 2 ** 31, 2, 2, 2) == (PLAIN, 0)


def test_ng_boundary_at_224_distinct_columns(pkg, lib):
    """ucap 224 takes 7 gather loads, 256 takes 10: one 64-row tile with exactly 224, then 225 distinct columns."""
    for u, ng in ((224, 7), (225, 10), (320, 10)):
        rp = np.arange(65, dtype=np.int64) * 5
        ci = np.sort((np.arange(320).reshape(64, 5) % u), axis=1).ravel()
        A = R.Csr(64, 400, rp, ci, np.ones(320))
        got = host_plan(pkg, lib, A)
        assert (got["umax"], got["ucap"], got["rows"]) == (u, (u + 31) // 32 * 32, (PAD, ng))
        assert got["rows"] == R.rows_route(R.plan(64, rp, ci), 400, 16, 16, 16)
    ci = np.arange(321, dtype=np.int64)                      # 321 distinct columns in one row: beyond every tile height
    A = R.Csr(1, 400, [0, 321], ci, np.ones(321))
    assert host_plan(pkg, lib, A)["state"] == -1 and R.plan(1, A.rowptr, ci)["state"] == -1


def test_column_major_route_boundaries(pkg, lib):
    for per, g in ((10, 8), (11, 16), (20, 16), (21, 32), (40, 32), (41, 64)):
        A = R.generate(100, 120, per, empty=())
        assert A.nnz == 100 * per
        for k in (1, 2, 5):
            got = host_plan(pkg, lib, A, k=k, ldx=k + (k & 1), ldy=k + (k & 1))
            want = 0 if k == 1 and got["tiles_ok"] else g
            assert got["cols"] == want == R.cols_route(A.nnz, 100, k, R.spmv_tiles_ok(100, A.rowptr)), (per, k)
    # just above each threshold by ONE entry in the whole matrix
    for per, g in ((10, 16), (20, 32), (40, 64)):
        A = R.generate(100, 120, per, empty=(), lengths=[per + 1] + [per] * 99)
        assert A.nnz == 100 * per + 1 and host_plan(pkg, lib, A, k=2)["cols"] == g == R.cols_route(A.nnz, 100, 2, True)
    # csr_spmv_tiles' capacity: a 64-row tile of exactly 2304 entries stays, 2305 goes to the lane group at k = 1
    for extra, ok in ((0, True), (1, False)):
        A = R.generate(100, 120, 36, empty=(), lengths=[36 + extra] + [36] * 63 + [3] * 36)
        assert A.rowptr[64] == 2304 + extra
        got = host_plan(pkg, lib, A, k=1, ldx=2, ldy=2)
        assert got["tiles_ok"] == ok == R.spmv_tiles_ok(100, A.rowptr)
        assert got["cols"] == (0 if ok else 32) == R.cols_route(A.nnz, 100, 1, ok)


def test_reference_bound_passes_float64_sums_and_catches_mutations():
    """The check the GPU tests apply, on the host: float64 sums in CSR order and in reversed order are inside the row-wise bound;
    a product with one entry of ONE short row dropped, with fp32-rounded values, or with one right-hand side's neighbour read
    instead is outside it -- also where that row is 1e-6 of the result's norm (what a whole-result tolerance passes)."""
    A = R.generate(100, 300, 17)
    X = np.random.default_rng(3).standard_normal((300, 6))
    X[A.unreferenced()] = np.nan
    A.vals[A.rowptr[40]:A.rowptr[41]] *= 1e-6                 # a row of small magnitude
    rows = A.rows()

    def product(vals, Xm, order=slice(None)):
        Y = np.zeros((100, Xm.shape[1]))
        for e in np.arange(A.nnz)[order]:
            Y[rows[e]] += vals[e] * Xm[A.colidx[e]]
        return Y
    Y = product(A.vals, X)
    assert R.check(Y, A, X) <= 1.0 and R.check(product(A.vals, X, slice(None, None, -1)), A, X) <= 1.0
    assert R.check(product(A.vals.astype(np.float32).astype(np.float64), X), A, X, f32=True) <= 1.0
    dropped = A.vals.copy()
    dropped[A.rowptr[40] + 3] = 0.0
    assert np.linalg.norm(product(dropped, X) - Y) < 1e-5 * np.linalg.norm(Y)      # invisible to a whole-result tolerance
    for wrong in (product(dropped, X), product(A.vals.astype(np.float32).astype(np.float64), X), product(A.vals, np.roll(X, 1, axis=1))):
        with pytest.raises(AssertionError):
            R.check(wrong, A, X)
    with pytest.raises(AssertionError):                      # a live cell never written keeps its (finite) sentinel
        Ys = Y.copy()
        Ys[5, 2] = -1.2345e300
        R.check(Ys, A, X)


# the instantiations the plan reaches WITHOUT the withhold flag on the generator's matrices (100 rows; DESIGN.md has the table)
REACHED_UNAIDED = {(PAD, 64, 7), (PAD, 64, 10), (PAD, 32, 7), (PAD, 32, 10), (PAD, 16, 7), (PAD, 16, 10), (TILES, 64, 7)}


def test_reachability_of_the_tiled_instantiations():
    """Search small generator settings for every (kernel, R, NG): which does the plan reach on its own?  The unpadded kernel runs
    only where its image fits 52 KB and the padded one does not fit 53 KB -- the padded image is the larger one only where rows pad
    heavily AND there are many entries, which the taller tiles of few distinct columns alone offer."""
    reached = {}
    for width in (48, 96, 160, 224, 300, 400, 700):
        for per in list(range(1, 48)) + [49, 57, 65, 73, 81, 89, 97, 105, 113, 121]:
            if per > width:
                continue
            A = R.generate(100, width, per)
            pl = R.plan(100, A.rowptr, A.colidx)
            kind, ng = R.rows_route(pl, width, 16, 16, 16)
            if kind != PLAIN:
                reached.setdefault((kind, pl["R"], ng), (width, per))
    print("reached unaided:", {k: reached[k] for k in sorted(reached)})
    assert set(reached) == REACHED_UNAIDED
